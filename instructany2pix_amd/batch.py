"""Batched, sharded serving of independent edit requests on the denoise hot path.

The reference serves one request at a time on one GPU (instructany2pix/pipeline.py:303-386; serve.py:115 serialises the queue), so every knob of
`__call__` -- `num_inference_steps`, `cfg`, `scale`, `alpha` (pipeline.py:303-304) -- is a per-call scalar. Independent requests share nothing
(GroupNorm / LayerNorm / attention are per sample), so this module runs N of them as ONE batch per UNet evaluation:

  * every batch element carries its own timestep (its own position in its own schedule), its own IP-Adapter scale and its own guidance scale:
    `ia2p_unet_forward_v` (timesteps[B], ip_scales[B]) and `ia2p_ddim_step_v` (per-request {g, c_x, c_e});
  * requests whose schedule is shorter simply stop moving (c_x = 1, c_e = 0) while the others finish;
  * across the GPUs of a node the request list is sharded contiguously (`dist.shard_range`), every rank runs its shard in groups (default 4
    requests = B_eff 8 in the guided sampling loop, the shape the headline metric is quoted on) and the results are all-gathered.

Per request the hot segment is the reference's: DDIM inversion of the base latents (pnp_pipeline.py:92-278, no guidance), polar mixing with fresh
noise on the CPU in fp16 (pipeline.py:331-337), IP-Adapter guided sampling (ip_adapter.py:289-356 -> sdxl_pipeline.py:764-857).
Batch element b of a heterogeneous batch gets the bits it gets in a uniform batch of the same size (tests/test_batch_gpu.py); against a
batch-1 run only the summation order of batch-dependent kernel plans differs (fp16 tolerance).

Layout of the module. The host code the serial pipelines also need lives with them and is called from here: `scheduler.kept_steps` (strength -> kept
tail), `ddim.conditioning` ([uncond | cond] context, pooled embeddings, time ids), `noise.host_noises` / `noise.resolve_noises` (supplied noise, then
seed, then generator), the request-level helpers of `pipeline.py`. Here:
  * tables: `invert_tables`, `sample_tables`, `refine_tables`, `inpaint_tables` give every request what its scheduler gives it alone, and `_joint_tables`
    lays them out `[iterations][requests]`, a request that is through HELD on its hold record;
  * one driver, `_run_groups` (shard, groups, concatenate, empty shard, all-gather), under `denoise_batch`, `refine_batch` and `inpaint_batch`, which
    validate and resolve the noises first;
  * three group bodies with their own launch loops, `_denoise_group` (`invert_batch`, mix, `sample_batch`), `_refine_group`, `_inpaint_group`: their
    buffer hand-offs differ (ping-pong through out2; x apart from the scaled input; `stepped` blended into both halves), so they are not one loop;
  * `edit_batch`: whole requests through all of it.
An edit inside a mask (`EditRequest.edit_mask`, `RefineRequest.known_latents` / `.edit_mask`, `edit_batch(edit_masks=)`): in a group where a request
has a mask, `invert_batch` records its trajectory through `out2` of its update launch, `sample_batch` follows the start and every iteration with one selection
launch at each request's own level (`scheduler.known_levels`, a table like the coefficient tables) and `_refine_group` blends the base latents in at the loop's
noise level; a group without masks runs the launch sequence it always ran.
Few-step sampling (`EditRequest.sampler` / `.sample_steps` / `.step_noise`, `edit_batch(samplers=, sample_steps=, sample_adapters=)`): a group holds one
sampler; under "lcm" `sample_batch` hands its rows to `lcm_sample`, the one loop of the consistency sampler (`lcm_tables`, `ia2p_lcm_step_v`), which the serial
pipeline calls too. With every such keyword at None nothing here launches or draws anything it did not before.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import dist as D
from . import noise as _noise
from .ddim import conditioning, get_add_time_ids
from .scheduler import (DDIMScheduler, LCMScheduler, check_kept_steps, check_step_noise, fused_update_v, kept_steps, known_blend_v, known_levels, lcm_update_v,
                        level_table, mask_blend_v, resolve_sampler)


@dataclass
class EditRequest:
    """One edit request on explicit conditioning (what `InstructAny2PixPipeline.denoise` takes), with its own knobs."""
    base_latents: torch.Tensor                 # [1, 4, h, w] x0 of the base image
    latent_la: torch.Tensor                    # [D] fused instruction embedding (IP-Adapter input, reference pipeline.py:322-324)
    prompt_embeds: torch.Tensor                # [1, 77, ctx]
    pooled_prompt_embeds: torch.Tensor         # [1, pooled]
    negative_prompt_embeds: torch.Tensor
    negative_pooled_prompt_embeds: torch.Tensor
    inv_prompt_embeds: Optional[torch.Tensor] = None      # embedding of '' (reference :330); default: the negative ones
    inv_pooled_prompt_embeds: Optional[torch.Tensor] = None
    alpha: float = 0.7
    num_inference_steps: int = 25
    cfg: float = 10.0
    scale: float = 1.0
    noise: Optional[torch.Tensor] = None       # polar-mixing noise (CPU fp16); None: drawn from the global RNG in request order
    seed: Optional[int] = None                 # the request's own Philox stream (noise.py): without `noise`, draw DRAW_POLAR of it, made and mixed on the device
    edit_mask: Optional[object] = None         # edit inside this mask only (what `pipeline.resolve_edit_mask` takes: a pixel mask, or a latent mask [1, 1, h, w])
    auto_mask: Optional[object] = None         # estimate the mask from the request itself (auto_mask.py: True, a dict or an AutoMask); times `edit_mask` where both are given
    sampler: Optional[str] = None              # "ddim" or "lcm"; None: what `pipe.pipe.scheduler` is (DDIM, or LCM when an `LCMScheduler` is assigned there)
    sample_steps: Optional[int] = None         # length of the LCM schedule (default 4, 1 .. 50); `num_inference_steps` keeps governing the inversion
    step_noise: Optional[torch.Tensor] = None  # LCM: the noise injected after every step but the last, fp16 [sample_steps - 1, 4, h, w]; wins over the seed (draw DRAW_LCM)
    subject_mode: str = "serial"               # the request's subject-consistency stage, serial or joint (`edit_batch(subject_modes=)` sets it; the hot segment does not read it)


def _coef_table(rows: Sequence[Sequence[tuple]], device) -> torch.Tensor:
    """a host table of the joint loop, float32 on the device: [steps][B] timesteps, [steps][B][3] (g, c_x, c_e) or [steps][B][2] (c0, c1) of every request"""
    return torch.tensor(rows, dtype=torch.float32).to(device).contiguous()


def _joint_tables(records: Sequence[Sequence[tuple]], hold: Sequence[tuple]) -> tuple:
    """The one layout of all four joint loops. `records[r]`: one tuple of fields per step of request r alone (its timestep, its coefficients, ...);
    `hold[r]`: the tuple it carries once it is through -- its last timestep and coefficients that keep its latents bit for bit. -> per field one
    `[iterations][requests]` table: every request starts at iteration 0, the shorter ones are padded with their hold record."""
    nmax = max(len(rec) for rec in records)
    rows = [[rec[k] if k < len(rec) else hold[r] for r, rec in enumerate(records)] for k in range(nmax)]
    return tuple([[cell[f] for cell in row] for row in rows] for f in range(len(hold[0])))


def invert_tables(scheduler_config, steps: Sequence[int]):
    """What `SDXLDDIMPipeline.inverse` gives every request alone over its own `steps[r]`-step schedule, walked in ascending t, laid out for the joint loop:
    -> (timesteps, coef). A live row is (0, *inversion_coeffs(abar_t, abar_prev)), the first step against `final_alpha_cumprod` (pnp_pipeline.py:262-267);
    a held row is (0, 1, 0) at the request's last timestep. Pure host arithmetic: needs no GPU."""
    records, hold = [], []
    for n in steps:
        sch = DDIMScheduler.from_config(scheduler_config)
        sch.set_timesteps(n)
        acp, asc = sch.alphas_cumprod, [int(t) for t in reversed(sch.timesteps)]
        prev = [float(sch.final_alpha_cumprod)] + [float(acp[t]) for t in asc[:-1]]
        records.append([(float(t), (0.0,) + DDIMScheduler.inversion_coeffs(float(acp[t]), a_prev)) for t, a_prev in zip(asc, prev)])
        hold.append((float(asc[-1]), (0.0, 1.0, 0.0)))
    return _joint_tables(records, hold)


def sample_tables(scheduler_config, steps: Sequence[int], cfg: Sequence[float]):
    """What `StableDiffusionXLPipeline.__call__` gives every request alone over its own schedule, laid out for the joint loop: -> (timesteps, coef), the
    timesteps duplicated over both halves of [uncond x n | cond x n]. A live row is (cfg[r], *step_coeffs(t)); a held row is (0, 1, 0) at the request's last
    timestep (g = 0 here, where the refiner and inpaint loops hold with their g: with c_e = 0 the guidance never enters). Pure host arithmetic."""
    records, hold = [], []
    for n, g in zip(steps, cfg):
        sch = DDIMScheduler.from_config(scheduler_config)
        sch.set_timesteps(n)
        desc = [int(t) for t in sch.timesteps]
        records.append([(float(t), (float(g),) + sch.step_coeffs(t)) for t in desc])
        hold.append((float(desc[-1]), (0.0, 1.0, 0.0)))
    ts, coef = _joint_tables(records, hold)
    return [row + row for row in ts], coef


def lcm_tables(scheduler_config, steps: Sequence[int], cfg: Sequence[float], per: Optional[int] = None, seeded: Optional[Sequence[bool]] = None):
    """What `LCMScheduler` gives every request alone over its own `steps[r]`-step LCM schedule, laid out for the joint loop: -> (timesteps, coef, firsts),
    each `[iterations][requests]` (the caller repeats a timestep row for the two halves of a guided evaluation). A live row is (cfg[r], *step_coeffs(s)) =
    (g, c_x, c_e, c_n) at the request's own timestep; a held row is (0, 1, 0, 0) at its last timestep. `firsts` is what `ia2p_lcm_step_v` takes: for a
    request with seeded[r] (and `per` elements per request) at its step s the element `noise.lcm_first(s, per)` of draw DRAW_LCM its step noise starts at;
    -1 for a held row and for a request whose noise comes by pointer. Pure host arithmetic."""
    records, hold = [], []
    seeded = [False] * len(steps) if seeded is None or per is None else [bool(s) for s in seeded]
    for n, g, own in zip(steps, cfg, seeded):
        sch = LCMScheduler.from_config(scheduler_config)
        sch.set_timesteps(int(n))
        desc = [int(t) for t in sch.timesteps]
        records.append([(float(t), (float(g),) + sch.step_coeffs(s), _noise.lcm_first(s, per) if own else -1) for s, t in enumerate(desc)])
        hold.append((float(desc[-1]), (0.0, 1.0, 0.0, 0.0), -1))
    return _joint_tables(records, hold)


def lcm_blend_tables(scheduler_config, steps: Sequence[int]):
    """The re-noising of the base latents outside an edit mask after every LCM step, `[iterations][requests]` in the (c0, c1) form of `ia2p_mask_blend_v`:
    (sqrt(p), sqrt(1 - p)) at the timestep the step arrives at, (1, 0) after a request's last step and while it is held."""
    records = []
    for n in steps:
        sch = LCMScheduler.from_config(scheduler_config)
        sch.set_timesteps(int(n))
        records.append([(sch.renoise_coeffs(s),) for s in range(int(n))])
    return _joint_tables(records, [((1.0, 0.0),)] * len(records))[0]


@torch.no_grad()
def lcm_sample(unet, scheduler_config, x, ctx, added, steps: Sequence[int], cfg: Sequence[float], guided: bool, step_noise=None, seeds=None, ip_scales=None,
               base=None, edit_mask=None, unet_kw=None, callback=None):
    """The loop of the consistency sampler, serial (`ddim.StableDiffusionXLPipeline.__call__` under an `LCMScheduler`) and batched (`sample_batch`): x [n, 4, h, w]
    on the device -> x0, request r over its own `steps[r]`-step LCM schedule (`lcm_tables`). `guided`: one evaluation at 2 n rows [uncond x n | cond x n] and
    eps_u + g (eps_c - eps_u) per iteration; else the n conditional rows alone and eps_c = NULL (`ctx`, `added`, `ip_scales` come laid out accordingly).
    The noise injected after step s of request r: `step_noise[r]` [steps[r] - 1, 4, h, w] read by pointer, else draw DRAW_LCM of `seeds[r]` made inside the
    update launch -- a request with more than one step has one of the two.
    `base` + `edit_mask` (an edit inside a mask): each step's result is replaced, where the mask is 0, by sqrt(p) base + sqrt(1 - p) z with the z of the step
    itself (`ia2p_mask_blend_v`; (1, 0) after the last step: the base latents' bits). The step noise of an iteration is then materialised first
    (`randn_seeded(first = s P)` for the seeded rows) and the step reads it by pointer."""
    dev, n = x.device, x.shape[0]
    per = x.numel() // n
    steps = [int(s) for s in steps]
    step_noise = [None] * n if step_noise is None else list(step_noise)
    seeds = [None] * n if seeds is None else list(seeds)
    for r in range(n):
        if step_noise[r] is not None:
            check_step_noise(step_noise[r], steps[r], x.shape, f" (request {r})")
        elif seeds[r] is None and steps[r] > 1:
            raise ValueError(f"request {r} takes {steps[r]} LCM steps and has neither `step_noise` nor a seed to draw it from")
    own = [r for r in range(n) if step_noise[r] is None and seeds[r] is not None]
    masked = edit_mask is not None
    if masked != (base is not None):
        raise ValueError("`base` and `edit_mask` go together: pass both or neither")
    ts, coef, firsts = lcm_tables(scheduler_config, steps, cfg, per, [r in own and not masked for r in range(n)])
    ts_all, coef_all = _coef_table([row + row for row in ts] if guided else ts, dev), _coef_table(coef, dev)
    noise_all = None
    if masked or len(own) < n:                  # rows that read their noise by pointer: [iterations, n, 4, h, w], zeros where no noise is injected
        noise_all = torch.zeros((len(ts),) + tuple(x.shape), dtype=torch.float16, device=dev)
        for r, z in enumerate(step_noise):
            if z is not None and steps[r] > 1:
                noise_all[:steps[r] - 1, r] = z.to(dev)
    if masked:
        blend_all = _coef_table(lcm_blend_tables(scheduler_config, steps), dev)
    cs, draws = [0 if s is None else _noise.check_seed(s) for s in seeds], [_noise.DRAW_LCM] * n
    model_in = torch.cat([x, x], dim=0).contiguous() if guided else x.clone()
    eps, nxt = torch.empty_like(model_in), torch.empty_like(model_in)
    for i in range(len(ts)):
        unet(model_in, ts_all[i], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps, ip_scales=ip_scales, **(unet_kw or {}))
        cur, eps_u, eps_c, out2 = model_in[:n], eps[:n], (eps[n:] if guided else None), (nxt[n:] if guided else None)
        if not masked:
            if noise_all is not None:
                z = noise_all[i]
            else:                               # every row is seeded; a held row (first -1) carries c_n = 0, so the pointer it is given is never read
                z = cur if min(firsts[i]) < 0 else None
            lcm_update_v(cur, eps_u, eps_c, coef_all[i], nxt[:n], out2, noise=z, seeds=cs, draws=draws, firsts=firsts[i])
        else:
            z = noise_all[i]
            if own:
                z[own] = _noise.randn_seeded([cs[r] for r in own], _noise.DRAW_LCM, x.shape[1:], torch.float16, dev, first=_noise.lcm_first(i, per))
            lcm_update_v(cur, eps_u, eps_c, coef_all[i], nxt[:n], noise=z)
            mask_blend_v(nxt[:n], base, z, edit_mask, blend_all[i], nxt[:n], out2)
        model_in, nxt = nxt, model_in
        if callback is not None:
            callback(i, ts[i][0], model_in[:n])
    return model_in[:n].clone()


def _shard(N: int, shard: bool):
    """(world, lo, hi): the contiguous shard [lo, hi) of N requests this rank runs (`dist.shard_range`); everything when `shard` is off or no process group is up"""
    world = torch.distributed.get_world_size() if (shard and torch.distributed.is_available() and torch.distributed.is_initialized()) else 1
    rank = torch.distributed.get_rank() if world > 1 else 0
    return (world,) + D.shard_range(N, world, rank)


def _gather_shards(t: torch.Tensor, N: int, world: int) -> torch.Tensor:
    """every rank's shard rows [n_r, ...] -> all N rows in request order on every rank (equal-sized shards for the all-gather: pad, gather, cut)"""
    if world == 1:
        return t
    per = (N + world - 1) // world
    pad = torch.zeros((per,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[: t.shape[0]] = t
    allr = D.gather_batches(pad).reshape(world, per, *t.shape[1:])
    return torch.cat([allr[r][: D.shard_range(N, world, r)[1] - D.shard_range(N, world, r)[0]] for r in range(world)], dim=0)


def _run_groups(requests: list, like: torch.Tensor, unet, group: int, shard: bool, run_group, n_out: int = 1):
    """The driver of the three batch functions: this rank's contiguous shard of the (validated) requests in groups of `group`, `run_group(g0, reqs)` -> a
    tuple of `n_out` tensors [len(reqs), ...] for the group that starts at request g0; per output, the groups' rows concatenated (an empty shard gives
    [0, ...] of `like`'s shape) and all-gathered -> a tuple of `n_out` tensors [N, ...] in request order on every rank."""
    N = len(requests)
    world, lo, hi = _shard(N, shard)
    outs = [run_group(g0, requests[g0:min(g0 + group, hi)]) for g0 in range(lo, hi, group)]
    empty = torch.empty((0,) + tuple(like.shape[1:]), dtype=torch.float16, device=unet.device)
    return tuple(_gather_shards(torch.cat([o[j] for o in outs]) if outs else empty, N, world) for j in range(n_out))


def _rows(xs: Sequence[torch.Tensor], device) -> torch.Tensor:
    """the requests' [1, ...] tensors as the [n, ...] rows of their group, fp16 on the device"""
    return torch.cat([x.to(device=device, dtype=torch.float16) for x in xs], dim=0).contiguous()


def _check_group(group, what: str):
    if not 1 <= int(group) <= 8:
        raise ValueError(f"group={group}: a group is one launch sequence of 1..8 requests (B_eff = 2 * group <= 16 rows, the limit of the image-projection and "
                         f"embedding kernels) -- {what}")


def _check_latents(latents: Sequence[torch.Tensor], what: str):
    if len(latents) == 0:
        raise ValueError(f"{what} needs at least one request")
    shapes = {tuple(x.shape[-2:]) for x in latents}
    if len(shapes) != 1:
        raise ValueError(f"requests of one call must share the latent size, got {sorted(shapes)}")


@torch.no_grad()
def invert_batch(unet, scheduler_config, latents, prompt_embeds, pooled, steps: Sequence[int], ip_scales=None, return_trajectory: bool = False):
    """DDIM inversion x0 -> xT of B requests at once (reference loop pnp_pipeline.py:251-275 per request), each over its own `steps[b]`-step
    schedule walked in ascending t (`invert_tables`). latents [B,4,h,w]; prompt_embeds [B,L,ctx]; pooled [B,P].
    `return_trajectory` (False: nothing changes): -> (xT, trajectory fp16 [max(steps) + 1, B, 4, h, w]), level 0 the latents the loop starts from, level
    j + 1 the result of iteration j, written through `out2` of the update launch (no extra launch). A request that is through is held: its levels above
    its own N repeat its xT and are never read (`scheduler.known_levels`)."""
    dev = unet.device
    x = latents.to(device=dev, dtype=torch.float16).contiguous().clone()
    h, w = x.shape[-2] * 8, x.shape[-1] * 8
    ctx, added = conditioning(dev, prompt_embeds, pooled, get_add_time_ids(unet, (h, w), (0, 0), (h, w), int(pooled.shape[-1])))      # unguided
    ts, coef = invert_tables(scheduler_config, steps)
    ts_all, coef_all = _coef_table(ts, dev), _coef_table(coef, dev)
    eps, nxt = torch.empty_like(x), torch.empty_like(x)
    traj = None
    if return_trajectory:
        traj = torch.empty((len(ts) + 1,) + tuple(x.shape), dtype=torch.float16, device=dev)
        traj[0].copy_(x)
    for i in range(len(ts)):
        unet(x, ts_all[i], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps, ip_scales=ip_scales)
        if traj is None:
            fused_update_v(x, eps, None, coef_all[i], nxt)
        else:
            fused_update_v(x, eps, None, coef_all[i], nxt, traj[i + 1])
        x, nxt = nxt, x
    return x if traj is None else (x, traj)


@torch.no_grad()
def sample_batch(unet, scheduler_config, latents, cond_ctx, uncond_ctx, cond_pooled, uncond_pooled, steps: Sequence[int], cfg: Sequence[float],
                 scales: Optional[Sequence[float]] = None, known: Optional[torch.Tensor] = None, edit_mask: Optional[torch.Tensor] = None, sampler: Optional[str] = None,
                 step_noise=None, seeds=None, base: Optional[torch.Tensor] = None):
    """Guided DDIM sampling xT -> x0 of n requests at once: one UNet evaluation at B_eff = 2 n per iteration, rows [uncond x n | cond x n]
    (the reference's cat([latents] * 2), sdxl_pipeline.py:826, per request), request r with its own schedule length, guidance and IP scale
    (`sample_tables`).
    `known` + `edit_mask` (both None: nothing changes): mask-guided decoding. `known` is `invert_batch(return_trajectory=True)`'s store over the same
    `steps`, `edit_mask` the {0, 1} latent masks [n, 1, h, w] (all ones for a request without a mask: the selection returns its bits). Where a mask is 0 the
    start is the request's level N_r and the result of iteration i its level max(N_r - 1 - i, 0) (`scheduler.known_levels`, uploaded once next to the
    coefficient tables): one `ia2p_known_blend_v` launch per iteration, written to both halves of the model input.
    `sampler` (None or "ddim": nothing changes) = "lcm": the consistency sampler. `steps` are then the lengths of the requests' LCM schedules and the update is
    `ia2p_lcm_step_v` (`lcm_sample`: `step_noise`, `seeds`, and `base` + `edit_mask` for an edit inside a mask -- `known` has no use there). When every
    request has cfg <= 1 the group runs without guidance, on its n conditional rows; a group that mixes cfg <= 1 with cfg > 1 is refused."""
    if sampler not in (None, "ddim", "lcm"):
        raise ValueError(f"sampler must be 'ddim', 'lcm' or None, got {sampler!r}")
    lcm = sampler == "lcm"
    if not lcm and (step_noise is not None or base is not None):
        raise ValueError("`step_noise` and `base` belong to sampler='lcm'")
    guided = not (lcm and all(float(g) <= 1.0 for g in cfg))
    if lcm and guided and any(float(g) <= 1.0 for g in cfg):
        raise ValueError("LCM requests with cfg <= 1 (no guidance: conditional rows only) and with cfg > 1 cannot share a call")
    dev = unet.device
    n = latents.shape[0]
    x = latents.to(device=dev, dtype=torch.float16).contiguous()
    h, w = x.shape[-2] * 8, x.shape[-1] * 8
    ctx, added = conditioning(dev, cond_ctx, cond_pooled, get_add_time_ids(unet, (h, w), (0, 0), (h, w), int(cond_pooled.shape[-1])),
                              *((uncond_ctx, uncond_pooled) if guided else ()))
    if lcm:
        if known is not None:
            raise ValueError("the LCM timesteps are not the inversion's levels: pass `base`, not `known`")
        sc = None if scales is None else torch.tensor(list(scales) * (2 if guided else 1), dtype=torch.float32).to(dev)
        if base is not None:
            base = base.to(device=dev, dtype=torch.float16).contiguous()
        return lcm_sample(unet, scheduler_config, x, ctx, added, steps, cfg, guided, step_noise, seeds, sc, base, edit_mask)
    ts, coef = sample_tables(scheduler_config, steps, cfg)
    ts_all, coef_all = _coef_table(ts, dev), _coef_table(coef, dev)
    sc = None
    if scales is not None:
        sc = torch.tensor(list(scales) * 2, dtype=torch.float32).to(dev)
    lv = None
    if (known is None) != (edit_mask is None):
        raise ValueError("`known` and `edit_mask` go together: pass both or neither")
    if known is not None:
        if tuple(known.shape) != (len(ts) + 1,) + tuple(x.shape) or tuple(edit_mask.shape) != (n, 1) + tuple(x.shape[-2:]):
            raise ValueError(f"`known` must be [max(steps) + 1 = {len(ts) + 1}, {', '.join(map(str, x.shape))}] and `edit_mask` [{n}, 1, {x.shape[-2]}, {x.shape[-1]}], "
                             f"got {tuple(known.shape)} and {tuple(edit_mask.shape)}")
        lv = level_table(known_levels(steps), known.shape[0], dev)
        x = known_blend_v(x, known, lv[0], edit_mask, torch.empty_like(x))
    model_in = torch.cat([x, x], dim=0).contiguous()
    eps, nxt = torch.empty_like(model_in), torch.empty_like(model_in)
    for i in range(len(ts)):
        unet(model_in, ts_all[i], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps, ip_scales=sc)
        if lv is None:
            fused_update_v(model_in[:n], eps[:n], eps[n:], coef_all[i], nxt[:n], nxt[n:])    # eps_u + g (eps_c - eps_u), x_{t-1} to both halves
        else:                                                                                # outside the masks: the inverted latents of each request's level
            fused_update_v(model_in[:n], eps[:n], eps[n:], coef_all[i], nxt[:n])
            known_blend_v(nxt[:n], known, lv[i + 1], edit_mask, nxt[:n], nxt[n:])
        model_in, nxt = nxt, model_in
    return model_in[:n].clone()


@torch.no_grad()
def _denoise_group(pipeline, reqs: List[EditRequest], noises, masks=None, lcm=None, sample_adapters=None):
    """one group through inversion, polar mixing and guided sampling -> (sampled latents, inverted latents). `noises[i]` None: request i mixes on the device
    with draw DRAW_POLAR of its own stream. `masks[i]`: request i's latent edit mask [1, 1, h, w] or None; with at least one mask in the group the inversion
    records its trajectory and the sampling is mask-guided, the requests without one carrying all ones. Without any, the launch sequence is the unmasked one.
    `lcm` (None: a DDIM group): per request (length of its LCM schedule, its step noise or None for a seeded request) -- the guided sampling runs the
    consistency sampler (`sample_batch(sampler="lcm")`); an edit mask then needs no trajectory, the base latents themselves are re-noised outside it.
    `sample_adapters`: (names, weights) active on the UNet around the guided sampling loop only (`LoraManager.using`)."""
    from . import pipeline as P                  # (`polar_intrtpolate` looked up at call time)
    unet, cfgs, ipa = pipeline.pipe.unet, pipeline.pipe.scheduler.config, pipeline.ip_adapter_xl
    dev = unet.device
    steps = [int(r.num_inference_steps) for r in reqs]
    cat = lambda xs: torch.cat([x.to(dev) for x in xs], dim=0)
    inv_ctx = cat([(r.inv_prompt_embeds if r.inv_prompt_embeds is not None else r.negative_prompt_embeds) for r in reqs])
    inv_pool = cat([(r.inv_pooled_prompt_embeds if r.inv_pooled_prompt_embeds is not None else r.negative_pooled_prompt_embeds) for r in reqs])
    guided = {}
    if masks is not None and any(m is not None for m in masks):
        hw = tuple(reqs[0].base_latents.shape[-2:])
        guided["edit_mask"] = torch.cat([torch.ones((1, 1) + hw, dtype=torch.float16, device=dev) if m is None else m.to(device=dev, dtype=torch.float16)
                                         for m in masks], dim=0).contiguous()
        if lcm is None:
            x_inv, guided["known"] = invert_batch(unet, cfgs, cat([r.base_latents for r in reqs]), inv_ctx, inv_pool, steps, return_trajectory=True)
        else:
            guided["base"] = cat([r.base_latents for r in reqs])
            x_inv = invert_batch(unet, cfgs, guided["base"], inv_ctx, inv_pool, steps)
    else:
        x_inv = invert_batch(unet, cfgs, cat([r.base_latents for r in reqs]), inv_ctx, inv_pool, steps)
    own = [i for i in range(len(reqs)) if noises[i] is None]
    if len(own) < len(reqs):
        x_inv_cpu = x_inv.cpu()                                                             # pipeline.py:331
    if not own:
        mixed = torch.cat([P.polar_intrtpolate(x_inv_cpu[i:i + 1], noises[i].to(x_inv_cpu.dtype), r.alpha) for i, r in enumerate(reqs)], dim=0)
    else:                            # seeded rows: noise and mix on the device, one launch each over those rows; the latents never leave it
        z = _noise.randn_seeded([reqs[i].seed for i in own], _noise.DRAW_POLAR, x_inv.shape[1:], torch.float16, dev)
        mixed = torch.empty_like(x_inv)
        mixed[own] = _noise.polar_mix(x_inv[own] if len(own) < len(reqs) else x_inv, z, [float(reqs[i].alpha) for i in own])
        for i, r in enumerate(reqs):
            if noises[i] is not None:
                mixed[i:i + 1] = P.polar_intrtpolate(x_inv_cpu[i:i + 1], noises[i].to(x_inv_cpu.dtype), r.alpha).to(dev)
    ip, ip_un = ipa.get_image_embeds(clip_image_embeds=torch.stack([r.latent_la.reshape(-1) for r in reqs]), mode="global")
    cond_ctx = torch.cat([cat([r.prompt_embeds for r in reqs]).to(torch.float16), ip], dim=1)              # ip_adapter.py:341-342
    uncond_ctx = torch.cat([cat([r.negative_prompt_embeds for r in reqs]).to(torch.float16), ip_un], dim=1)
    if lcm is not None:
        steps = [n for n, _ in lcm]
        guided.update(sampler="lcm", step_noise=[z for _, z in lcm], seeds=[r.seed for r in reqs])
    with (contextlib.nullcontext() if sample_adapters is None else unet.lora.using(*sample_adapters)):
        x = sample_batch(unet, cfgs, mixed, cond_ctx, uncond_ctx, cat([r.pooled_prompt_embeds for r in reqs]), cat([r.negative_pooled_prompt_embeds for r in reqs]),
                         steps, [float(r.cfg) for r in reqs], [float(r.scale) for r in reqs], **guided)
    return x, x_inv


def resolve_sample_adapters(unet, sample_adapters):
    """`sample_adapters=` -> None or (names, weights) for `LoraManager.using`: a name, a list of names (weight 1 each) or (names, weights). An adapter that
    is not loaded is refused here, before any launch."""
    if sample_adapters is None:
        return None
    names, weights = sample_adapters if isinstance(sample_adapters, tuple) else (sample_adapters, 1.0)
    names = [names] if isinstance(names, str) else list(names)
    if not names:
        raise ValueError("sample_adapters names no adapter")
    weights = [float(weights)] * len(names) if not isinstance(weights, (list, tuple)) else [float(w) for w in weights]
    if len(weights) != len(names):
        raise ValueError(f"sample_adapters: {len(names)} adapter names for {len(weights)} weights")
    loaded = list(unet.lora.adapters) if getattr(unet, "_lora", None) is not None else []
    for nm in names:
        if nm not in loaded:
            raise ValueError(f"sample_adapters: no adapter '{nm}' is loaded (loaded: {loaded})")
    return names, weights


def lcm_plan(scheduler, requests):
    """per request ("ddim", None) or ("lcm", length of its LCM schedule) (`scheduler.resolve_sampler`), with the refusals that need no model: `sample_steps`
    under DDIM, a `step_noise` of the wrong shape or under DDIM, LCM requests with cfg <= 1 next to LCM requests with cfg > 1"""
    plan = [resolve_sampler(scheduler, r.sampler, r.sample_steps, f" (request {i})") for i, r in enumerate(requests)]
    for i, (r, (smp, n)) in enumerate(zip(requests, plan)):
        if r.step_noise is not None:
            if smp != "lcm":
                raise ValueError(f"`step_noise` is the noise of the LCM sampler; request {i} samples with DDIM")
            check_step_noise(r.step_noise, n, r.base_latents.shape, f" (request {i})")
    g = [float(r.cfg) <= 1.0 for r, (smp, _) in zip(requests, plan) if smp == "lcm"]
    if any(g) and not all(g):
        raise ValueError("LCM requests with cfg <= 1 (no guidance: conditional rows only) and with cfg > 1 cannot share a call")
    return plan


@torch.no_grad()
def denoise_batch(pipeline, requests: List[EditRequest], group: int = 4, shard: bool = True, sample_adapters=None):
    """N independent edit requests through the hot segment, batched and (with an initialised process group) sharded over the ranks.
    Returns (sampled latents [N,4,h,w], inverted latents [N,4,h,w]) in request order on every rank.
    `group` requests share one launch sequence (B_eff = 2 * group under guidance): 4 is the headline shape; with a queue of requests 8 is 16 %
    cheaper per image (2.05 vs 2.44 ms per image-step, profiles/r03j_two_stream_probe.txt) at twice the latency of a group.
    A request with a `seed` (and no `noise`) takes its mixing noise from its own Philox stream (noise.py, draw DRAW_POLAR) and is mixed on the device
    (`ia2p_polar_mix_v`: fp32, not the bits of the CPU fp16 mix): its inverted latents never leave the device, its result does not depend on the requests around
    it, and no rank needs to be seeded alike for it. Requests without a seed draw and mix as ever, also next to seeded ones in one group.
    A request with `sampler="lcm"` (or None under an assigned `LCMScheduler`) is sampled by the consistency sampler over `sample_steps` steps
    after the same inversion and mixing; its step noise is `step_noise`, else draw DRAW_LCM of its seed made inside the update launch, else `sample_steps - 1`
    host draws right after its own polar-mixing draw. A group holds one sampler: a call that mixes samplers runs the DDIM requests' groups, then the LCM
    requests', each in request order. LCM requests with cfg <= 1 run without guidance (n rows per evaluation); all LCM requests of a call must agree on that.
    `sample_adapters`: a name, a list or (names, weights) -- LoRA adapters active around the guided sampling loops only."""
    latents = [r.base_latents for r in requests]
    _check_latents(latents, "denoise_batch")
    if pipeline.ip_adapter_xl is None:
        raise NotImplementedError("denoise_batch drives the IP-Adapter path (construct the pipeline with ip_ckpt=)")
    plan = lcm_plan(getattr(getattr(pipeline, "pipe", None), "scheduler", None), requests)
    if sample_adapters is not None:
        sample_adapters = resolve_sample_adapters(pipeline.pipe.unet, sample_adapters)
    for r, (smp, _) in zip(requests, plan):
        if r.num_inference_steps is None or int(r.num_inference_steps) <= 0:
            raise ValueError(f"`num_inference_steps` has to be a positive integer but is {r.num_inference_steps}")
        if smp == "ddim" and float(r.cfg) <= 1.0:
            # the reference (and pipeline.denoise) switch guidance OFF at guidance_scale <= 1 -- one conditional evaluation, eps = eps_c (sdxl_pipeline.py:842-844
            # behind do_classifier_free_guidance) -- while a batched group always evaluates [uncond | cond] and blends: not the same numbers. Say so instead.
            raise ValueError(f"denoise_batch blends eps_u + g (eps_c - eps_u) for every request; cfg={r.cfg} <= 1 means NO guidance in the reference: run that request "
                             f"through pipeline.denoise / __call__ instead")
    _check_group(group, "denoise_batch")
    if any(r.auto_mask is not None for r in requests):      # the mask estimates come first: their host draws precede every polar-mixing draw
        from .auto_mask import apply_auto_masks
        requests = apply_auto_masks(pipeline, requests, group)
    # polar-mixing noise comes from the global CPU RNG in REQUEST order (what N sequential reference calls would draw), on every rank alike; a request with a
    # seed and no noise draws nothing here: its noise is made on the device in its group, from its own stream
    lcm_idx = [i for i, (smp, _) in enumerate(plan) if smp == "lcm"]
    if not lcm_idx:
        noises = _noise.host_noises([r.noise for r in requests], [x.shape for x in latents], [r.seed for r in requests])
    else:                            # an unseeded LCM request draws its step noise right after its own polar-mixing noise, in step order: what N serial calls draw
        noises, step_noises = [], []
        for r, x, (smp, n) in zip(requests, latents, plan):
            noises += _noise.host_noises([r.noise], [x.shape], [r.seed])
            z = r.step_noise
            if smp == "lcm" and z is None and r.seed is None and n > 1:
                z = torch.cat([torch.randn(tuple(x.shape), dtype=torch.float16) for _ in range(n - 1)], dim=0)
            step_noises.append(z)
    masks = None
    if any(r.edit_mask is not None for r in requests):
        from .pipeline import resolve_edit_mask
        masks = [None if r.edit_mask is None else resolve_edit_mask(pipeline, r.edit_mask, r.base_latents, pixels=False)[1] for r in requests]      # every refusal before any launch
    extra = {} if sample_adapters is None else {"sample_adapters": sample_adapters}

    def run(idx, lcm):
        """the requests `idx` (one sampler) in groups -> (sampled, inverted) in their order"""
        sub = lambda xs, g0, k: [xs[i] for i in idx[g0:g0 + k]]
        kw = lambda g0, k: dict(extra, **({"lcm": [(plan[i][1], step_noises[i]) for i in idx[g0:g0 + k]]} if lcm else {}))
        if masks is None:
            return _run_groups([requests[i] for i in idx], latents[0], pipeline.pipe.unet, group, shard,
                               lambda g0, reqs: _denoise_group(pipeline, reqs, sub(noises, g0, len(reqs)), **kw(g0, len(reqs))), n_out=2)
        return _run_groups([requests[i] for i in idx], latents[0], pipeline.pipe.unet, group, shard,
                           lambda g0, reqs: _denoise_group(pipeline, reqs, sub(noises, g0, len(reqs)), sub(masks, g0, len(reqs)), **kw(g0, len(reqs))), n_out=2)
    if not lcm_idx or len(lcm_idx) == len(requests):
        return run(list(range(len(requests))), bool(lcm_idx))
    ddim_idx = [i for i in range(len(requests)) if i not in lcm_idx]
    parts = {False: run(ddim_idx, False), True: run(lcm_idx, True)}
    place = {i: (False, j) for j, i in enumerate(ddim_idx)}
    place.update({i: (True, j) for j, i in enumerate(lcm_idx)})
    return tuple(torch.cat([parts[place[i][0]][o][place[i][1]:place[i][1] + 1] for i in range(len(requests))], dim=0) for o in range(2))


# ---- the stages after the hot segment, batched the same way: refiner pass and subject-consistency inpainting ---------------------------------------------
# Row layout of every guided evaluation: [uncond x n | cond x n] (the reference's cat([latents] * 2) per request). All requests of a group start at
# iteration 0 at their own first kept timestep; a request with fewer steps is through early and is HELD: evaluated at its last timestep, moved with
# (g, 1, 0) (and, in the inpaint loop, blended with (1, 0)), which returns its latents bit for bit while the others finish.

def _kept_steps(num_inference_steps: int, strength: float, request: int):
    """`scheduler.kept_steps` with the serial pipelines' two refusals, naming the request"""
    if strength < 0 or strength > 1:
        raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength} (request {request})")
    t_start, n_steps = kept_steps(num_inference_steps, strength)
    check_kept_steps(n_steps, strength, f" (request {request})")
    return t_start, n_steps


def _check_loop_args(num_inference_steps, guidance_scale, what: str):
    if num_inference_steps is None or not isinstance(num_inference_steps, int) or num_inference_steps <= 0:
        raise ValueError(f"`num_inference_steps` has to be a positive integer but is {num_inference_steps} of type {type(num_inference_steps)}.")
    if float(guidance_scale) <= 1.0:
        raise ValueError(f"{what} blends eps_u + g (eps_c - eps_u) for every request; guidance_scale={guidance_scale} <= 1 means NO guidance in the serial "
                         f"pipeline: run such a request through it instead")


@dataclass
class RefineRequest:
    """One refiner pass on explicit conditioning (what `StableDiffusionXLImg2ImgPipeline.__call__(latents=...)` takes), with its own strength."""
    latents: torch.Tensor                      # [1, 4, h, w] clean latents, scaled
    prompt_embeds: torch.Tensor                # the four refiner embeddings (text encoder 2)
    pooled_prompt_embeds: torch.Tensor
    negative_prompt_embeds: torch.Tensor
    negative_pooled_prompt_embeds: torch.Tensor
    strength: float = 0.3
    noise: Optional[torch.Tensor] = None       # start noise; None: drawn from the global CPU RNG in request order
    seed: Optional[int] = None                 # without `noise`: draw DRAW_REFINER of the request's own stream, on the device
    known_latents: Optional[torch.Tensor] = None   # with `edit_mask`: [1, 4, h, w] kept (re-noised with the loop's own noise) where the mask is 0
    edit_mask: Optional[torch.Tensor] = None       # {0, 1} latent mask [1, 1, h, w]


@dataclass
class RefineTables:
    """Host tables of one group's joint Euler loop: `[iterations][requests]`, every coefficient triple in the (g, c_x, c_e) form of `ia2p_ddim_step_v`."""
    steps: List[int]                 # steps each request takes
    start_sigma: List[float]         # add_noise: x = latents + sigma * noise
    timesteps: List[List[float]]
    input_scale: List[List[float]]   # scale_model_input: 1 / sqrt(sigma^2 + 1)
    coef: List[List[tuple]]          # (g, 1, sigma_next - sigma); (g, 1, 0) once a request is through
    blend: List[List[tuple]]         # an edit inside a mask: (1, sigma_next), the known region at the noise level the step arrives at; (1, 0) after the last step and while held


def refine_tables(scheduler_config, strengths: Sequence[float], num_inference_steps: int = 50, guidance_scale: float = 5.0) -> RefineTables:
    """What `EulerDiscreteScheduler` gives every request alone (img2img.py: `get_timesteps` tail, `add_noise` sigma, `input_scale` / `step_coeffs` at index
    t_start + k), laid out for the joint loop. Pure host arithmetic: needs no GPU."""
    from .scheduler import EulerDiscreteScheduler
    sch = EulerDiscreteScheduler.from_config(scheduler_config)
    sch.set_timesteps(num_inference_steps)
    kept = [_kept_steps(num_inference_steps, float(s), i) for i, s in enumerate(strengths)]
    g = float(guidance_scale)
    records = [[(float(sch.timesteps[i]), sch.input_scale(i), (g,) + tuple(sch.step_coeffs(i)), (1.0, float(sch.sigmas[i + 1]))) for i in range(t_start, t_start + n)]
               for t_start, n in kept]
    hold = [rec[-1][:2] + ((g, 1.0, 0.0), (1.0, 0.0)) for rec in records]
    return RefineTables([n for _, n in kept], [float(sch.sigmas[sch.index_for_timestep(sch.timesteps[t_start])]) for t_start, _ in kept],
                        *_joint_tables(records, hold))


@torch.no_grad()
def _refine_group(piperf, reqs: List[RefineRequest], noises, tb: RefineTables, aesthetic_score, negative_aesthetic_score):
    from .img2img import get_add_time_ids_aesthetic
    unet = piperf.unet
    dev, n = unet.device, len(reqs)
    lat, noise = _rows([r.latents for r in reqs], dev), _rows(noises, dev)
    size = (lat.shape[-2] * piperf.vae_scale_factor, lat.shape[-1] * piperf.vae_scale_factor)
    ids, neg_ids = get_add_time_ids_aesthetic(unet, size, (0, 0), size, aesthetic_score, negative_aesthetic_score, size, (0, 0), size,
                                              int(reqs[0].pooled_prompt_embeds.shape[-1]), piperf.config.requires_aesthetics_score)
    ctx, added = conditioning(dev, _rows([r.prompt_embeds for r in reqs], dev), _rows([r.pooled_prompt_embeds for r in reqs], dev), ids,
                              _rows([r.negative_prompt_embeds for r in reqs], dev), _rows([r.negative_pooled_prompt_embeds for r in reqs], dev), neg_ids)
    ts_all = _coef_table([row + row for row in tb.timesteps], dev)
    scale_all = _coef_table([[(1.0, s, 0.0) for s in row] for row in tb.input_scale], dev)
    coef_all = _coef_table(tb.coef, dev)
    x, nxt = torch.empty_like(lat), torch.empty_like(lat)
    fused_update_v(lat, noise, None, _coef_table([(1.0, 1.0, s) for s in tb.start_sigma], dev), x)              # add_noise at every request's first kept timestep
    mask = None
    if any(r.edit_mask is not None for r in reqs):       # an edit inside a mask: outside it the known latents at the loop's noise level, with the loop's own noise
        if any((r.edit_mask is None) != (r.known_latents is None) for r in reqs):
            raise ValueError("`known_latents` and `edit_mask` of a RefineRequest go together: give both or neither")
        ones = torch.ones((1, 1) + tuple(lat.shape[-2:]), dtype=torch.float16, device=dev)
        mask = torch.cat([ones if r.edit_mask is None else r.edit_mask.to(device=dev, dtype=torch.float16) for r in reqs], dim=0).contiguous()
        known = _rows([r.latents if r.known_latents is None else r.known_latents for r in reqs], dev)          # (a row of ones keeps its x: the value is not used)
        if mask.shape != (n, 1) + tuple(lat.shape[-2:]) or known.shape != lat.shape:
            raise ValueError(f"every request carries ONE latent mask [1, 1, h, w] and known latents of its latents' shape, got {tuple(mask.shape)} and {tuple(known.shape)}")
        blend_all = _coef_table(tb.blend, dev)
        mask_blend_v(x, known, noise, mask, _coef_table([(1.0, s) for s in tb.start_sigma], dev), x)
    model_in = torch.empty((2 * n,) + tuple(x.shape[1:]), dtype=torch.float16, device=dev)
    eps = torch.empty_like(model_in)
    for k in range(len(tb.timesteps)):
        fused_update_v(x, x, None, scale_all[k], model_in[:n], model_in[n:])                                    # scale_model_input on cat([x] * 2)
        unet(model_in, ts_all[k], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps)
        fused_update_v(x, eps[:n], eps[n:], coef_all[k], nxt)                                                   # CFG + Euler step
        if mask is not None:
            mask_blend_v(nxt, known, noise, mask, blend_all[k], nxt)
        x, nxt = nxt, x
    return x


@torch.no_grad()
def refine_batch(piperf, requests: List[RefineRequest], group: int = 4, shard: bool = True, num_inference_steps: int = 50, guidance_scale: float = 5.0,
                 aesthetic_score: float = 6.0, negative_aesthetic_score: float = 2.5):
    """The refiner's Euler img2img loop (`StableDiffusionXLImg2ImgPipeline.__call__`, reference pipeline.py:358-361) for N requests: one UNet evaluation at
    B_eff = 2 n per iteration of a group, request r on its own `strength`-shortened tail of the shared 50-step schedule. The per-call values are the class
    defaults the reference runs with. -> refined latents [N, 4, h, w] in request order on every rank."""
    latents = [r.latents for r in requests]
    _check_latents(latents, "refine_batch")
    _check_group(group, "refine_batch")
    _check_loop_args(num_inference_steps, guidance_scale, "refine_batch")
    tables = lambda reqs: refine_tables(piperf.scheduler.config, [r.strength for r in reqs], num_inference_steps, guidance_scale)
    tables(requests)                                                                                           # every request's refusal before any launch
    noises = _noise.resolve_noises([r.noise for r in requests], [x.shape for x in latents], [r.seed for r in requests], [_noise.DRAW_REFINER] * len(requests),
                                   piperf.unet.device)
    return _run_groups(requests, latents[0], piperf.unet, group, shard, lambda g0, reqs: (_refine_group(
        piperf, reqs, noises[g0:g0 + len(reqs)], tables(reqs), aesthetic_score, negative_aesthetic_score),))[0]


@dataclass
class InpaintRequest:
    """One subject-consistency pass (what `IPAdapterXL(pipe_inpainting).generate(latents=, mask_image=, clip_image_embeds_local=, mode='local')` takes)."""
    latents: torch.Tensor                      # [1, 4, h, w] clean latents, scaled
    mask: torch.Tensor                         # anything `inpaint.prepare_mask` takes: 1 = repaint
    subject_embed: torch.Tensor                # [D] the subject's embedding ('local' crop of the image-projection model)
    prompt_embeds: torch.Tensor                # the four text embeddings of the pass (without image tokens)
    pooled_prompt_embeds: torch.Tensor
    negative_prompt_embeds: torch.Tensor
    negative_pooled_prompt_embeds: torch.Tensor
    strength: float = 0.7
    noise: Optional[torch.Tensor] = None       # start and re-noising noise; None: drawn from the global CPU RNG in request order
    seed: Optional[int] = None                 # without `noise`: draw `draw` of the request's own stream, on the device
    draw: int = _noise.DRAW_INPAINT            # DRAW_INPAINT + k for subject pass k
    # a JOINT pass over several subjects (regional image prompts: one loop, every subject's tokens under its own mask, the blend under their union): the
    # subjects' masks and embeddings as lists of equal length (1 .. 16); `mask` / `subject_embed` are then not read (pass None)
    masks: Optional[list] = None
    subject_embeds: Optional[list] = None


def pad_subjects(subjects: Sequence[tuple], h: int, w: int, device) -> tuple:
    """The padding rule of a joint group. `subjects`: per request (masks, embeddings), 1 .. 16 each -> (regions [n, G, h, w] fp16 in {0, 1}, embeddings
    [n G, D] fp16, G) with G the group's largest subject count: a request with fewer subjects is padded with ALL-ZERO masks and zero embeddings. A zero region weight
    puts a probability of exactly +0 into the attention's P.V product (`ia2p_attention_regions`), so the padding changes no bit of that row's result."""
    from .inpaint import prepare_mask
    G = max(len(m) for m, _ in subjects)
    if not 1 <= G <= 16 or any(len(m) != len(e) or len(m) < 1 for m, e in subjects):
        raise ValueError("a joint subject pass takes 1 .. 16 subjects per request, one embedding per mask")
    D = int(torch.as_tensor(subjects[0][1][0]).numel())
    regions = torch.zeros(len(subjects), G, h, w, dtype=torch.float16, device=device)
    embeds = torch.zeros(len(subjects), G, D, dtype=torch.float16, device=device)
    for r, (ms, es) in enumerate(subjects):
        for g, (m, e) in enumerate(zip(ms, es)):
            regions[r, g] = prepare_mask(m, h, w, device)[0, 0]
            embeds[r, g] = torch.as_tensor(e).reshape(-1).to(device=device, dtype=torch.float16)
    return regions, embeds.reshape(len(subjects) * G, D), G


@dataclass
class InpaintTables:
    """Host tables of one group's joint inpaint loop: `[iterations][requests]`."""
    steps: List[int]
    start: List[tuple]               # (1, c_x, c_e): x = c_x latents + c_e noise -- add_noise at the first kept timestep; (1, 0, init_noise_sigma) at strength 1.0
    timesteps: List[List[float]]
    coef: List[List[tuple]]          # (g, c_x, c_e) of DDIMScheduler.step; (g, 1, 0) once a request is through
    blend: List[List[tuple]]         # (c0, c1): add_noise to the NEXT timestep; (1, 0) after a request's last step and while it is held


def inpaint_tables(scheduler_config, strengths: Sequence[float], num_inference_steps: int = 50, guidance_scale: float = 7.5) -> InpaintTables:
    """What `DDIMScheduler` gives every request alone in inpaint.py's loop, laid out for the joint loop. Pure host arithmetic: needs no GPU."""
    sch = DDIMScheduler.from_config(scheduler_config)
    sch.set_timesteps(num_inference_steps)
    kept = [_kept_steps(num_inference_steps, float(s), i) for i, s in enumerate(strengths)]
    g, start, records = float(guidance_scale), [], []
    for (t_start, n), s in zip(kept, strengths):
        tail = [int(t) for t in sch.timesteps[t_start:]]
        start.append((1.0, 0.0, float(sch.init_noise_sigma)) if float(s) == 1.0 else (1.0,) + tuple(sch.add_noise_coeffs(tail[0])))
        blend = [tuple(sch.add_noise_coeffs(t)) for t in tail[1:]] + [(1.0, 0.0)]                    # no re-noising after the last step
        records.append([(float(t), (g,) + tuple(sch.step_coeffs(t)), b) for t, b in zip(tail, blend)])
    hold = [(rec[-1][0], (g, 1.0, 0.0), (1.0, 0.0)) for rec in records]
    return InpaintTables([n for _, n in kept], start, *_joint_tables(records, hold))


@torch.no_grad()
def _inpaint_group(ipa, reqs: List[InpaintRequest], noises, tb: InpaintTables, scale: float):
    from .inpaint import prepare_mask
    unet = ipa.pipe.unet
    dev, n = unet.device, len(reqs)
    lat, noise = _rows([r.latents for r in reqs], dev), _rows(noises, dev)
    h, w = lat.shape[-2:]
    regions = None
    if any(r.masks is not None for r in reqs):
        # a joint group: every request's subjects padded to the group's largest count (`pad_subjects`), their tokens [n, 4 G, ctx] from ONE image-projection
        # call, the blend under the union of each request's masks
        from .inpaint import union_mask
        regions, embeds, G = pad_subjects([(list(r.masks), list(r.subject_embeds)) if r.masks is not None else ([r.mask], [r.subject_embed]) for r in reqs], h, w, dev)
        mask = union_mask(regions).contiguous()
        ip, ip_un = ipa.get_image_embeds(clip_image_embeds_local=embeds, mode="local", scale_g=1.0, scale_l=0.5)
        ip, ip_un = ip.reshape(n, 4 * G, -1), ip_un.reshape(n, 4 * G, -1)
    else:
        mask = torch.cat([prepare_mask(r.mask, h, w, dev) for r in reqs], dim=0).contiguous()
        if tuple(mask.shape) != (n, 1, h, w):
            raise ValueError(f"every request carries ONE mask, got {tuple(mask.shape)} for {n} requests")
        # the subjects' 'local' image tokens, one call per group, with the crop weights IPAdapterXL.generate passes (scale_g = 1.0, scale_l = 0.5)
        ip, ip_un = ipa.get_image_embeds(clip_image_embeds_local=torch.stack([r.subject_embed.reshape(-1) for r in reqs]), mode="local", scale_g=1.0, scale_l=0.5)
    size = (h * ipa.pipe.vae_scale_factor, w * ipa.pipe.vae_scale_factor)
    ctx, added = conditioning(dev, torch.cat([_rows([r.prompt_embeds for r in reqs], dev), ip], dim=1), _rows([r.pooled_prompt_embeds for r in reqs], dev),
                              get_add_time_ids(unet, size, (0, 0), size, int(reqs[0].pooled_prompt_embeds.shape[-1])),
                              torch.cat([_rows([r.negative_prompt_embeds for r in reqs], dev), ip_un], dim=1),                 # ip_adapter.py:341-342
                              _rows([r.negative_pooled_prompt_embeds for r in reqs], dev))
    sc = torch.full((2 * n,), float(scale), dtype=torch.float32).to(dev)
    ts_all = _coef_table([row + row for row in tb.timesteps], dev)
    coef_all, blend_all = _coef_table(tb.coef, dev), _coef_table(tb.blend, dev)
    x = torch.empty_like(lat)
    fused_update_v(lat, noise, None, _coef_table(tb.start, dev), x)
    model_in = torch.cat([x, x], dim=0).contiguous()
    eps, stepped = torch.empty_like(model_in), torch.empty_like(x)
    kw = {} if regions is None else {"cross_attention_kwargs": {"ip_adapter_masks": torch.cat([regions, regions], dim=0).contiguous()}}      # both CFG rows: the same masks
    for k in range(len(tb.timesteps)):
        unet(model_in, ts_all[k], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps, ip_scales=sc, **kw)
        fused_update_v(model_in[:n], eps[:n], eps[n:], coef_all[k], stepped)
        mask_blend_v(stepped, lat, noise, mask, blend_all[k], model_in[:n], model_in[n:])
    return model_in[:n].clone()


@torch.no_grad()
def inpaint_batch(ipa, requests: List[InpaintRequest], group: int = 4, shard: bool = True, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                  scale: float = 0.8):
    """The inpaint DDIM loop (`StableDiffusionXLInpaintPipeline.__call__` behind `IPAdapterXL.generate(mode='local')`, reference gdino/lib.py:89-102) for N
    requests, one subject each: one UNet evaluation at B_eff = 2 n per iteration of a group, request r on its own `strength`-shortened tail of the shared
    schedule with its own mask and subject tokens. `ipa` is the adapter over the inpainting pipeline (`InstructAny2PixPipeline.ip_adapter_xl_inpaint`); steps,
    guidance and IP scale are what `subject_consistency` passes. The processors' own scale is left alone: the IP scale goes in per row.
    A request with `masks` / `subject_embeds` (lists) is a JOINT pass over its subjects; a group that holds one runs the regional route, every request padded
    to the group's largest subject count (`pad_subjects`: no bit of a row changes by it).
    -> latents [N, 4, h, w] in request order on every rank."""
    latents, unet = [r.latents for r in requests], ipa.pipe.unet
    _check_latents(latents, "inpaint_batch")
    _check_group(group, "inpaint_batch")
    _check_loop_args(num_inference_steps, guidance_scale, "inpaint_batch")
    tables = lambda reqs: inpaint_tables(ipa.pipe.scheduler.config, [r.strength for r in reqs], num_inference_steps, guidance_scale)
    tables(requests)                                                                                           # every request's refusal before any launch
    noises = _noise.resolve_noises([r.noise for r in requests], [x.shape for x in latents], [r.seed for r in requests], [r.draw for r in requests], unet.device)
    return _run_groups(requests, latents[0], unet, group, shard, lambda g0, reqs: (_inpaint_group(ipa, reqs, noises[g0:g0 + len(reqs)], tables(reqs), scale),))[0]


# ---- whole edit requests ---------------------------------------------------------------------------------------------------------------------------------

def per_request(value, N: int, name: str, is_one=None) -> list:
    """a knob of `__call__` as a scalar (for all requests) or a list of N"""
    one = is_one(value) if is_one is not None else not isinstance(value, (list, tuple))
    if one:
        return [value] * N
    if len(value) != N:
        raise ValueError(f"`{name}` has {len(value)} entries for {N} requests")
    return list(value)


def _is_one_h(v) -> bool:
    return len(v) == 3 and not any(isinstance(x, (list, tuple)) or (torch.is_tensor(x) and x.ndim > 0) for x in v)


def _vae_in_batches(pipeline, fn, t: torch.Tensor, group: int, decode: bool, seeds=None, draw: int = 0) -> torch.Tensor:
    """a VAE hook over [n, ...] in equal batches of at most `group` rows, and of no more than the attached VAE takes in one launch sequence at this size
    (`HipAutoencoderKL.max_batch`: at 1024 x 1024 a decode takes 3 images, an encode 7). `seeds` (encode with an attached VAE; entries None allowed): row i's
    posterior sample comes from draw `draw` of its own stream; a `vae_encode=` hook draws its own sample and sees no seed."""
    n, rows = t.shape[0], int(group)
    if pipeline.vae is not None:
        f = 1 if decode else pipeline.pipe.vae_scale_factor             # decode: latents in; encode: pixels in
        rows = min(rows, pipeline.vae.max_batch(t.shape[-2] // f, t.shape[-1] // f, decode))
    k = -(-n // rows)
    per = -(-n // k)
    if seeds is None or pipeline.vae is None or all(s is None for s in seeds):
        return torch.cat([fn(t[i:i + per]) for i in range(0, n, per)], dim=0)
    return torch.cat([fn(t[i:i + per], seeds=seeds[i:i + per], draw=draw) for i in range(0, n, per)], dim=0)


@torch.no_grad()
def edit_batch(pipeline, insts, mm_datas, *, alpha=0.7, h=(0.0, 0.4, 1.0), norm=20.0, refinement=0.5, num_inference_steps=25, subject_strength=0.0, cfg=10,
               scale=1.0, output_type="latent", debug=False, group: int = 4, shard: bool = True, seeds=None, edit_masks=None, edit_feather=8, auto_masks=None,
               lora_scale=None, samplers=None, sample_steps=None, sample_adapters=None, subject_modes="serial"):
    """`subject_modes` ("serial", "joint" or a list of N): a "joint" request repaints all its subjects in ONE inpaint stage (regional image prompts, one noise:
    draw DRAW_INPAINT + 0) -- not the serial result, where pass k + 1 starts from the repaint of pass k and draws its own noise. The serial requests of the call keep
    their bits. `InstructAny2PixPipeline.__call__` for N instructions on N images in one call -> the list of its `(non_refined, oo, msg)` tuples in request order.
    See `InstructAny2PixPipeline.edit_batch` for the contract (knobs, stages, RNG rule, sharding). `lora_scale`: one number for the whole call (a batch
    shares its weights: no per-request adapters); None launches nothing. `samplers`, `sample_steps` (a scalar or a list of N; None: as ever) and
    `sample_adapters` (one value per call): the consistency sampler for the guided sampling stage (`denoise_batch`)."""
    if lora_scale is not None:
        with pipeline.lora_scaled(lora_scale):
            return edit_batch(pipeline, insts, mm_datas, alpha=alpha, h=h, norm=norm, refinement=refinement, num_inference_steps=num_inference_steps,
                              subject_strength=subject_strength, cfg=cfg, scale=scale, output_type=output_type, debug=debug, group=group, shard=shard, seeds=seeds,
                              edit_masks=edit_masks, edit_feather=edit_feather, auto_masks=auto_masks, samplers=samplers, sample_steps=sample_steps,
                              sample_adapters=sample_adapters, subject_modes=subject_modes)
    from . import pipeline as P
    from .auto_mask import auto_mask_t_start, estimate_requests, intersect, resolve_auto_mask
    from .image_processor import requantize
    insts, mm_datas = list(insts), list(mm_datas)
    N = len(insts)
    if N == 0:
        raise ValueError("edit_batch needs at least one request")
    if len(mm_datas) != N:
        raise ValueError(f"{N} instructions for {len(mm_datas)} mm_data lists")
    P.check_output_type(pipeline, output_type)
    _check_group(group, "edit_batch")
    seeds = _noise.resolve_seeds(seeds, N)
    seeded = any(s is not None for s in seeds)
    edit_masks = per_request(edit_masks, N, "edit_masks")                 # one mask for all requests, or a list of N with None entries
    auto_masks = [resolve_auto_mask(a, f" (request {i})") for i, a in enumerate(per_request(auto_masks, N, "auto_masks"))]      # one value for all, or a list of N with None entries
    if any(m is not None for m in edit_masks) or any(a is not None for a in auto_masks):
        from .image_processor import check_edit_feather
        P.check_edit_output_type(output_type)
        edit_feather = check_edit_feather(edit_feather)
    alpha, norm, refinement = per_request(alpha, N, "alpha"), per_request(norm, N, "norm"), per_request(refinement, N, "refinement")
    steps, subject_strength = per_request(num_inference_steps, N, "num_inference_steps"), per_request(subject_strength, N, "subject_strength")
    cfg, scale, h = per_request(cfg, N, "cfg"), per_request(scale, N, "scale"), per_request(h, N, "h", _is_one_h)
    samplers, sample_steps = per_request(samplers, N, "samplers"), per_request(sample_steps, N, "sample_steps")
    subject_modes = per_request(subject_modes, N, "subject_modes")
    for i, m in enumerate(subject_modes):
        if m not in ("serial", "joint"):
            raise ValueError(f"subject_modes: 'serial' or 'joint', got {m!r} (request {i})")
    lcm = [False] * N
    sch = getattr(getattr(pipeline, "pipe", None), "scheduler", None)
    if any(v is not None for v in samplers + sample_steps) or isinstance(sch, LCMScheduler):
        lcm = [resolve_sampler(sch, samplers[i], sample_steps[i], f" (request {i})")[0] == "lcm" for i in range(N)]
        unguided = [float(cfg[i]) <= 1.0 for i in range(N) if lcm[i]]
        if any(unguided) and not all(unguided):
            raise ValueError("LCM requests with cfg <= 1 (no guidance: conditional rows only) and with cfg > 1 cannot share a call")
    if sample_adapters is not None:
        resolve_sample_adapters(pipeline.pipe.unet, sample_adapters)
    for i in range(N):
        if steps[i] is None or int(steps[i]) <= 0:
            raise ValueError(f"`num_inference_steps` has to be a positive integer but is {steps[i]} (request {i})")
        if float(cfg[i]) <= 1.0 and not lcm[i]:
            raise ValueError(f"edit_batch blends eps_u + g (eps_c - eps_u) for every request; cfg={cfg[i]} <= 1 (request {i}) means NO guidance in the "
                             f"reference: run that request through __call__ instead")
        if float(refinement[i]) > 0:
            _kept_steps(50, float(refinement[i]), i)
        if float(subject_strength[i]) > 0:
            _kept_steps(50, float(subject_strength[i]), i)
        if auto_masks[i] is not None:
            auto_mask_t_start(int(steps[i]), auto_masks[i].strength, f" (request {i})")
    if pipeline.ip_adapter_xl is None:
        raise NotImplementedError("edit_batch drives the IP-Adapter path (construct the pipeline with ip_ckpt=)")
    if pipeline.piperf is None and any(float(r) > 0 for r in refinement):
        raise ValueError("refinement > 0 needs the pipeline built with refiner_unet= (pass refinement=0 to serve these requests without the refiner pass)")

    # ---- conditioning: one LLM pass for all requests, or the conditioner per request; a request without <im_gen> is answered here -------------------------
    results: list = [None] * N
    cs = pipeline._conditions_for_batch(insts, mm_datas, seeds=seeds) if seeded else pipeline._conditions_for_batch(insts, mm_datas)
    for i, c in enumerate(cs):
        if c.get("image_embeds") is None:
            results[i] = (None, None, f"FAILED: the LLM produced no <im_gen>: {c.get('caption')!r}")
    live = [i for i in range(N) if results[i] is None]
    if not live:
        return results
    # the prior runs per request (reference :313-317)
    latent_la = {i: P.fuse_instruction_embedding(cs[i]["base_embed"], cs[i]["image_embeds"], P.prior_y0(pipeline, cs[i]), h[i], norm[i]) for i in live}

    # ---- base images -> latents, the images among them encoded in batches (posterior samples: global RNG, request order) -----------------------------------
    base = {i: cs[i]["base_latents"] for i in live if cs[i].get("base_latents") is not None}
    todo = [i for i in live if i not in base]
    base_px = {}                     # masked request -> its preprocessed base image, for the composite
    if todo:
        imgs = [P.base_image(pipeline, cs[i], f" (request {i})") for i in todo]                   # (every refusal before the image processor is touched)
        imgs = [pipeline.pipe_inversion.image_processor.preprocess(img) for img in imgs]
        base_px.update({i: t for i, t in zip(todo, imgs) if (edit_masks[i] is not None or auto_masks[i] is not None) and t.shape[1] != 4})
        enc = _vae_in_batches(pipeline, pipeline.pipe_inversion._vae_encode, torch.cat(imgs, dim=0), group, False,
                              seeds=[seeds[i] for i in todo], draw=_noise.DRAW_BASE_POSTERIOR)
        base.update({i: enc[j:j + 1] for j, i in enumerate(todo)})
    _check_latents([base[i] for i in live], "edit_batch")
    # edit masks: (pixel mask, latent mask) per masked request, every refusal before the hot segment
    edit = {i: P.resolve_edit_mask(pipeline, edit_masks[i], base[i], P.edit_mask_file_size(cs[i])) for i in live if edit_masks[i] is not None}
    edit_m = {i: (edit[i][1] if i in edit else None) for i in live}

    # ---- the hot segment ---------------------------------------------------------------------------------------------------------------------------------
    reqs = [EditRequest(base_latents=base[i], latent_la=latent_la[i].reshape(1, -1)[0], **P.embeds(cs[i]), inv_prompt_embeds=cs[i].get("inv_prompt_embeds"),
                        inv_pooled_prompt_embeds=cs[i].get("inv_pooled_prompt_embeds"), alpha=alpha[i], num_inference_steps=int(steps[i]), cfg=float(cfg[i]),
                        scale=float(scale[i]), noise=cs[i].get("polar_noise"), seed=seeds[i], edit_mask=edit_m[i], auto_mask=auto_masks[i], sampler=samplers[i],
                        sample_steps=sample_steps[i], step_noise=cs[i].get("step_noise"), subject_mode=subject_modes[i]) for i in live]
    pipeline.pipe_inversion.unet = pipeline.pipe.unet
    # automatic masks, before the inversion: the estimate times the user's latent mask is the request's edit mask from here on; its pixel mask is
    # the latent mask's cells, inside the user's pixel mask where there is one
    auto = {}
    if any(r.auto_mask is not None for r in reqs):
        for j, (i, e) in enumerate(zip(live, estimate_requests(pipeline, reqs, group=group))):
            if e is None:
                continue
            auto[i] = e
            px, m = P.resolve_edit_mask(pipeline, intersect(e.mask, edit_m[i]), base[i])
            edit[i] = (torch.minimum(px, edit[i][0]) if i in edit else px, m)
            edit_m[i] = m
            reqs[j].edit_mask, reqs[j].auto_mask = m, None
    images, latent_inv = denoise_batch(pipeline, reqs, group=group, shard=shard, **({} if sample_adapters is None else {"sample_adapters": sample_adapters}))
    row = {i: j for j, i in enumerate(live)}
    non_refined = {i: images[row[i]:row[i] + 1] for i in live}
    oo = dict(non_refined)
    decoded = {}                     # request -> the decode of its `non_refined`, when the refiner hand-over made it

    # ---- refiner pass for the requests that ask for it -----------------------------------------------------------------------------------------------------
    ref = [i for i in live if float(refinement[i]) > 0]
    if ref:
        for i in ref:
            P._need(cs[i], P.REFINER_KEYS, "refiner pass")
        piperf = pipeline.piperf
        start = torch.cat([non_refined[i] for i in ref], dim=0)
        if P.refiner_handoff_by_image(pipeline):     # the reference's hand-over: decode, 8-bit image, re-encode (a posterior SAMPLE: global RNG, request order)
            dec = _vae_in_batches(pipeline, pipeline.pipe._vae_decode, start, group, True)
            decoded.update({i: dec[j:j + 1] for j, i in enumerate(ref)})
            img8 = requantize(dec) if pipeline.vae is not None else P.to_8bit_image(dec)
            start = _vae_in_batches(pipeline, piperf._vae_encode, img8, group, False, seeds=[seeds[i] for i in ref], draw=_noise.DRAW_HANDOFF_POSTERIOR)
        rr = [RefineRequest(latents=start[j:j + 1], **P.embeds(cs[i], "refiner_"), strength=float(refinement[i]), noise=cs[i].get("refiner_noise"), seed=seeds[i],
                            known_latents=base[i] if i in edit else None, edit_mask=edit_m[i]) for j, i in enumerate(ref)]
        refined = refine_batch(piperf, rr, group=group, shard=shard)
        oo.update({i: refined[j:j + 1] for j, i in enumerate(ref)})

    # ---- subject consistency: every request's masks first, then pass k over the requests with more than k subjects ---------------------------------------
    sub = [i for i in live if float(subject_strength[i]) > 0 and len(cs[i].get("subject_data") or []) > 0]
    if sub:
        pairs = {}
        for i in sub:
            P._need(cs[i], P.SUBJECT_KEYS, "subject-consistency pass")
            pairs[i] = pipeline._subject_mask_pairs(cs[i], cs[i]["subject_data"], oo[i])
            if i in edit:                                                                          # a subject pass under an edit mask repaints inside both
                pairs[i] = [(P.intersect_subject_mask(mk, edit[i][0]), emb) for mk, emb in pairs[i]]
        joint = [i for i in sub if subject_modes[i] == "joint"]
        if joint:                    # one inpaint stage for the joint requests: all subjects of a request in one loop, one noise
            ir = [InpaintRequest(latents=oo[i], mask=None, subject_embed=None, masks=[mk for mk, _ in pairs[i]], subject_embeds=[emb for _, emb in pairs[i]],
                                 **P.embeds(cs[i], "subject_"), strength=float(subject_strength[i]), noise=cs[i].get("subject_noise"), seed=seeds[i],
                                 draw=_noise.inpaint_draw(0)) for i in joint]
            painted = inpaint_batch(pipeline.ip_adapter_xl_inpaint, ir, group=group, shard=shard)
            oo.update({i: painted[j:j + 1] for j, i in enumerate(joint)})
        sub = [i for i in sub if subject_modes[i] != "joint"]
        for k in range(max([len(pairs[i]) for i in sub], default=0)):
            now = [i for i in sub if len(pairs[i]) > k]
            ir = [InpaintRequest(latents=oo[i], mask=pairs[i][k][0], subject_embed=pairs[i][k][1], **P.embeds(cs[i], "subject_"), strength=float(subject_strength[i]),
                                 noise=cs[i].get("subject_noise"), seed=seeds[i], draw=_noise.inpaint_draw(k)) for i in now]
            painted = inpaint_batch(pipeline.ip_adapter_xl_inpaint, ir, group=group, shard=shard)
            oo.update({i: painted[j:j + 1] for j, i in enumerate(now)})

    # ---- results; every latent is decoded once ----------------------------------------------------------------------------------------------------------
    shown_nr, shown_oo = dict(non_refined), dict(oo)
    if output_type != "latent":
        post = pipeline.pipe.image_processor.postprocess
        want = [(i, False) for i in live if i not in decoded] + [(i, True) for i in live if oo[i] is not non_refined[i]]
        if want:
            dec = _vae_in_batches(pipeline, pipeline.pipe._vae_decode, torch.cat([(oo if final else non_refined)[i] for i, final in want], dim=0), group, True)
        imgs = {key: dec[j:j + 1] for j, key in enumerate(want)}
        if edit:                     # the masked requests' base images in 8 bits (the loaded image, or the decode of the base latents) and feathered masks
            from .image_processor import image_to_u8, mask_feather
            need = [i for i in edit if i not in base_px]
            if need:
                dec_base = _vae_in_batches(pipeline, pipeline.pipe._vae_decode, _rows([base[i] for i in need], pipeline.pipe.unet.device), group, True)
                base_px.update({i: dec_base[j:j + 1] for j, i in enumerate(need)})
            base_u8 = {i: image_to_u8(base_px[i].to(torch.float16).contiguous()) for i in edit}
            alpha_u8 = {i: mask_feather(edit[i][0], edit_feather) for i in edit}
        for i in live:
            show = (lambda x, i=i: P.composite_edit(pipeline, x, base_u8[i], alpha_u8[i])) if i in edit else (lambda x: post(x, output_type=output_type))
            shown_nr[i] = show(decoded[i] if i in decoded else imgs[(i, False)])
            shown_oo[i] = shown_nr[i] if oo[i] is non_refined[i] else show(imgs[(i, True)])
    for i in live:
        msg = "SUCCESS!" if not debug else dict(output_caption=cs[i]["caption"], latent_inv=latent_inv[row[i]:row[i] + 1], latent_la=latent_la[i],
                                                **({} if seeds[i] is None else {"seed": seeds[i]}), **({} if i not in edit else {"edit_mask_latent": edit_m[i]}),
                                                **({} if i not in auto else {"edit_mask": edit_m[i], "auto_mask_map": auto[i].map, "auto_mask_stats": auto[i].stats}))
        results[i] = (shown_nr[i], shown_oo[i], msg)
    return results
