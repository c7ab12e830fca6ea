"""Seeded normal draws of an edit request, made on the device (include/ia2p.h, "Seeded noise"; csrc/noise.hip).

A request has a 64-bit seed; each of its normal draws has a draw id (the constants below). A value depends on (seed, draw id, flat element index inside the
request's own tensor) only -- not on the requests that share a launch, their order, the group size or the rank that computes it -- so a request gets the
same noise alone and in any batch. The same seed also keys the request's token stream under the LLM's device sampler (`generate_batch(seeds=)`): the two
domains never share a Philox block (the last counter word tells them apart).

  randn_seeded(seeds, draws, shape, dtype, device)   one tensor [len(seeds), *shape] of standard normals, row b from stream (seeds[b], draws[b])
  posterior_sample(moments, seeds, draw, scaling)    the VAE posterior sample `DiagonalGaussianDistribution.sample() * scaling_factor` from such a draw
  polar_mix(x, y, alphas)                            the reference's `polar_intrtpolate` (pipeline.py:295-300) per request, in fp32 on the device
  seeds_from_global(n)                               n fresh seeds from torch's global CPU generator, as the LLM's device sampler draws its own
  lcm_first(s, per)                                  where the step noise of the consistency sampler starts in draw DRAW_LCM (drawn inside `ia2p_lcm_step_v`)

`polar_mix` is the arithmetic of the seeded path only: fp32 sums and one rounding to fp16 at the end. It is NOT bit-equal to the CPU fp16 tensor arithmetic
of `pipeline.polar_intrtpolate`, which the unseeded path keeps.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _ffi

DRAW_BASE_POSTERIOR = 0        # VAE posterior sample of the base image
DRAW_POLAR = 1                 # polar-mixing noise (reference pipeline.py:335)
DRAW_HANDOFF_POSTERIOR = 2     # posterior sample of the refiner hand-off's re-encode
DRAW_REFINER = 3               # refiner start noise
DRAW_INPAINT = 4               # + k: inpaint noise of subject pass k (k < 65 532: below the next id)
DRAW_AUTO_MASK = 1 << 16       # the n noises of an automatic edit mask (auto_mask.py): element k * per + e is element e of noise k
DRAW_LCM = (1 << 16) + 1         # step noise of the consistency sampler: the noise injected after step s is elements s * P .. s * P + per - 1, P = per rounded up to 4


def lcm_first(s: int, per: int) -> int:
    """the first element of draw DRAW_LCM that the noise injected after step s of a request's own schedule starts at (a multiple of 4: a whole Philox block)"""
    return int(s) * (-(-int(per) // 4) * 4)


def inpaint_draw(k: int) -> int:
    """the draw id of subject pass k"""
    return DRAW_INPAINT + int(k)


def check_seed(seed) -> int:
    s = int(seed)
    if isinstance(seed, bool) or s < 0 or s >= 2 ** 64:
        raise ValueError(f"a seed is a 64-bit unsigned integer, got {seed!r}")
    return s


def check_draw(draw) -> int:
    d = int(draw)
    if d < 0 or d >= 2 ** 32:
        raise ValueError(f"a draw id is a 32-bit unsigned integer, got {draw!r}")
    return d


def resolve_seeds(seeds, n: int) -> list:
    """`edit_batch(seeds=)`: None -> [None] * n (today's draws); one int s -> s + i for request i (wrapping at 2^64); a list of n -> itself, entries None
    or a seed"""
    if seeds is None:
        return [None] * n
    if isinstance(seeds, int) and not isinstance(seeds, bool):
        return [(check_seed(seeds) + i) % 2 ** 64 for i in range(n)]
    seeds = list(seeds)
    if len(seeds) != n:
        raise ValueError(f"{len(seeds)} seeds for {n} requests: one per request")
    return [None if s is None else check_seed(s) for s in seeds]


def batch_seeds(noise_seed, batch: Optional[int]) -> list:
    """`noise_seed=` of the serial pipelines for a batch of `batch` rows (None: one row): an int s -> s + b for row b, a list -> one per row"""
    if isinstance(noise_seed, (list, tuple)):
        seeds = [check_seed(s) for s in noise_seed]
        if batch is not None and len(seeds) != batch:
            raise ValueError(f"{len(seeds)} noise seeds for a batch of {batch}")
        return seeds
    return [(check_seed(noise_seed) + b) % 2 ** 64 for b in range(1 if batch is None else batch)]


def seeds_from_global(n: int) -> list:
    """n seeds as 63-bit draws from torch's global CPU generator, in request order (`torch.manual_seed` fixes them): what the LLM's device sampler does when
    it is given none (llm.py `_resolve_seeds`)"""
    return [int(torch.randint(0, 2 ** 63 - 1, (1,)).item()) for _ in range(int(n))]


def _rows(seeds: Sequence[int], draws) -> tuple:
    seeds = [check_seed(s) for s in seeds]
    n = len(seeds)
    if n < 1:
        raise ValueError("at least one seed")
    draws = [check_draw(draws)] * n if isinstance(draws, int) else [check_draw(d) for d in draws]
    if len(draws) != n:
        raise ValueError(f"{n} seeds, {len(draws)} draw ids")
    return n, (C.c_uint64 * n)(*seeds), (C.c_uint32 * n)(*draws)


@torch.no_grad()
def randn_seeded(seeds: Sequence[int], draws, shape, dtype=torch.float16, device="cuda:0", first: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Standard normals [len(seeds), *shape] on `device` (`ia2p_randn_seeded`): row b holds elements first .. first + prod(shape) - 1 of the stream
    (seeds[b], draws[b]); `draws` is one id for every row or a list. dtype float32 (the rule's own values) or float16 (their round-to-nearest-even).
    `out`: a contiguous device tensor of that many elements to write instead of allocating."""
    n, cs, cd = _rows(seeds, draws)
    shape = tuple(int(s) for s in shape)
    per = 1
    for s in shape:
        per *= s
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"randn_seeded writes float16 or float32, not {dtype}")
    if out is None:
        out = torch.empty((n,) + shape, dtype=dtype, device=device)
    elif out.dtype != dtype or out.numel() != n * per:
        raise ValueError(f"out: {out.numel()} elements of {out.dtype} for {n} x {per} of {dtype}")
    if not out.is_cuda:
        raise _ffi.IA2PError("randn_seeded draws on an MI355X device (no CPU path exists)")
    with torch.cuda.device(out.device):
        _ffi.check(_ffi.lib().ia2p_randn_seeded(_ffi.current_stream(), _ffi.ptr(out), int(dtype == torch.float16), n, per, int(first), cs, cd))
    return out


def host_noises(given, shapes, seeds, generator=None) -> list:
    """The first two steps of the start-noise rule, per item (a request of a batch, or the whole batch of a serial call): a supplied tensor wins; an item
    with a seed is left None (its noise is made on the device, `resolve_noises` or the caller's own launch) and draws NOTHING here; every other item draws
    fp16 normals of its `shapes[i]` from `generator` (one, or a list whose first counts), else from torch's global CPU generator -- in item order, which
    is what serial calls one after the other draw, on every rank alike."""
    g = generator[0] if isinstance(generator, list) else generator
    gen_dev = g.device if g is not None else torch.device("cpu")
    return [n if n is not None or s is not None else torch.randn(tuple(shape), generator=g, device=gen_dev, dtype=torch.float16)
            for n, shape, s in zip(given, shapes, seeds)]


def resolve_noises(given, shapes, seeds, draws, device, generator=None) -> list:
    """The start-noise rule of the serial pipelines and the batched loops: supplied `noise`, then the seed, then `generator` or the global RNG.
    `seeds[i]`: None, an int (row b of the item draws from seed + b) or one seed per row (`batch_seeds`); `draws[i]`: the item's draw id. All host draws
    come first (`host_noises`); the seeded items then share ONE `randn_seeded` launch on `device`."""
    out = host_noises(given, shapes, seeds, generator)
    own = [i for i, n in enumerate(out) if n is None]
    if own:
        rows = [batch_seeds(seeds[i], shapes[i][0]) for i in own]
        ids = draws[own[0]] if len(own) == 1 else [draws[i] for i, r in zip(own, rows) for _ in r]      # (one item: one id for all its rows)
        z = randn_seeded([s for r in rows for s in r], ids, tuple(shapes[own[0]][1:]), torch.float16, device)
        for i, zi in zip(own, z.split([len(r) for r in rows])):
            out[i] = zi
    return out


@torch.no_grad()
def posterior_sample(moments: torch.Tensor, seeds: Sequence[int], draw, scaling_factor: float) -> torch.Tensor:
    """`DiagonalGaussianDistribution(moments).sample() * scaling_factor` with the normals of stream (seeds[b], draw) (`ia2p_posterior_sample_seeded`):
    moments fp16 [B, 2 C, h, w] on the device as `HipAutoencoderKL.encode` leaves them -> fp16 [B, C, h, w]"""
    if moments.ndim != 4 or moments.shape[1] % 2 or moments.dtype != torch.float16:
        raise ValueError(f"moments must be fp16 [B, 2 C, h, w], got {tuple(moments.shape)} {moments.dtype}")
    moments = moments.contiguous()
    B, C2, h, w = moments.shape
    n, cs, cd = _rows(seeds, draw)
    if n != B:
        raise ValueError(f"{n} seeds for {B} images: one per image")
    out = torch.empty(B, C2 // 2, h, w, dtype=torch.float16, device=moments.device)
    with torch.cuda.device(moments.device):
        _ffi.check(_ffi.lib().ia2p_posterior_sample_seeded(_ffi.current_stream(), _ffi.ptr(moments), _ffi.ptr(out), B, C2 // 2, h * w, float(scaling_factor), cs, cd))
    return out


@torch.no_grad()
def polar_mix(x: torch.Tensor, y: torch.Tensor, alphas) -> torch.Tensor:
    """`polar_intrtpolate(x[b], y[b], alphas[b])` for every row of x, y (fp16 [B, ...] on the device) in one launch (`ia2p_polar_mix_v`): norms and the mixture
    in fp32, one rounding to fp16. `alphas`: one float or one per row. Not the bits of the CPU fp16 arithmetic of the unseeded path (module docstring)."""
    for t in (x, y):
        if t.dtype != torch.float16 or not t.is_cuda:
            raise ValueError("polar_mix takes fp16 device tensors")
    if x.shape != y.shape or x.ndim < 1:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must have one shape [B, ...]")
    x, y = x.contiguous(), y.contiguous()
    B = x.shape[0]
    alphas = [float(alphas)] * B if not isinstance(alphas, (list, tuple)) else [float(a) for a in alphas]
    if len(alphas) != B:
        raise ValueError(f"{len(alphas)} alphas for {B} rows")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _ffi.check(_ffi.lib().ia2p_polar_mix_v(_ffi.current_stream(), _ffi.ptr(x), _ffi.ptr(y), (C.c_float * B)(*alphas), _ffi.ptr(out), B, x.numel() // max(B, 1)))
    return out
