"""Automatic edit masks on the MI355X (C ABI: ia2p_eps_contrast_map, ia2p_contrast_mask; host: instructany2pix_amd/auto_mask.py).

The kernels against the fp64 reference of tests/auto_mask_ref.py: exact on lattice inputs, within the derived bound on real-valued ones, the mask equal on every
decision-certain cell. The loops promise bit identity: the estimate equals its stages composed by hand from the same launches, `auto_mask=` equals `edit_mask=<that mask>`,
and outside the mask the result is the base latents / the base image's bytes. Tiny configs, 16 x 16 latents, 3 to 5 steps (tests/test_edit_batch_gpu.py's models)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import auto_mask_ref as R                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(tgt, src, ratio=3.0, dilate=1):
    """numpy [B, n, C, h, w] -> (map, stats, mask) from the two launches, as numpy"""
    from instructany2pix_amd.auto_mask import contrast_map, contrast_mask
    cmap = contrast_map(torch.from_numpy(np.ascontiguousarray(tgt)).to(DEV), torch.from_numpy(np.ascontiguousarray(src)).to(DEV))
    mask, stats = contrast_mask(cmap, ratio, dilate)
    torch.cuda.synchronize()
    return cmap.cpu().numpy(), stats.cpu().numpy(), mask.cpu().numpy()


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.LATTICE_CASES)
def test_lattice_cases_equal_the_reference_exactly(shape):
    tgt, src = R.lattice_case(*shape, seed=7)
    for d in (0, 1):
        cmap, stats, _, mask = R.auto_mask_ref(tgt, src, 3.0, d)
        got_map, got_stats, got_mask = _run(tgt, src, 3.0, d)
        assert np.array_equal(got_map.astype(np.float64), cmap) and np.array_equal(got_stats.astype(np.float64), stats)
        assert got_mask.dtype == np.float16 and np.array_equal(got_mask, mask)
        assert d or 0.1 < mask.mean() < 0.5


@pytest.mark.parametrize("n,C,h,w", [(2, 4, 8, 8), (8, 4, 16, 16), (2, 4, 64, 64)])
def test_ties_at_tau_are_off(n, C, h, w):
    tgt, src = R.tie_case(n, C, h, w)
    cmap, stats, m, mask = R.auto_mask_ref(tgt, src, 3.0, 0)
    assert (cmap == stats[0, 1]).sum() == 3 * h * w // 8                             # the case does hold ties
    got_map, got_stats, got_mask = _run(tgt, src, 3.0, 0)
    assert np.array_equal(got_map.astype(np.float64), cmap) and got_stats.tolist() == [[0.5, 0.75]] and np.array_equal(got_mask, mask)
    assert got_mask.sum() == h * w // 8
    same = np.ones((1, n, C, h, w), np.float16)                                      # equal predictions: mean 0, an empty mask, nothing non-finite
    got_map, got_stats, got_mask = _run(same, same, 3.0, 2)
    assert not got_map.any() and got_stats.tolist() == [[0.0, 0.0]] and not got_mask.any()


@pytest.mark.parametrize("i,shape", list(enumerate(R.REAL_CASES)))
def test_real_valued_cases_are_within_the_derived_bound(i, shape):
    B, n, C, h, w = shape
    tgt, src = R.real_case(*shape, seed=100 + i)
    cmap, stats, m, _ = R.auto_mask_ref(tgt, src, 3.0, 0)
    got_map, got_stats, got_mask = _run(tgt, src, 3.0, 0)
    bm, bmean, btau = R.bounds(cmap, stats, n * C)
    err = np.abs(got_map - cmap)
    print(f"map err / bound max {np.max(err / np.maximum(bm, 1e-300)):.3f}; mean {np.abs(got_stats[:, 0] - stats[:, 0]) / bmean}; tau {np.abs(got_stats[:, 1] - stats[:, 1]) / btau}")
    assert (err <= bm).all()
    assert (np.abs(got_stats[:, 0] - stats[:, 0]) <= bmean).all() and (np.abs(got_stats[:, 1] - stats[:, 1]) <= btau).all()
    sure = R.certain(cmap, stats, n * C)
    assert ((~sure).reshape(B, -1).sum(axis=1) <= R.max_uncertain(h * w)).all()      # a condition on the case, not a tolerance
    assert np.array_equal(got_mask[:, 0][sure] != 0, m[sure])
    dil = R.auto_mask_ref(tgt, src, 3.0, 2)[3]                                       # the dilated mask, where every cell of the window is certain
    got_dil = _run(tgt, src, 3.0, 2)[2]
    window_sure = ~R.dilate_ref(~sure, 2)
    assert np.array_equal(got_dil[:, 0][window_sure], dil[:, 0][window_sure])


@pytest.mark.parametrize("HW", [63, 64, 65])
def test_a_request_has_the_same_bits_alone_and_as_row_two_of_three(HW):
    """placement: its place in the launch, B, and the base pointers' alignment (row 2 of 3 at HW = 63 / 65 starts off the 16-byte grid; an odd element offset into a
    larger buffer moves every base off it) change nothing"""
    from instructany2pix_amd.auto_mask import contrast_map, contrast_mask
    n, C = 3, 4
    tgt, src = R.real_case(3, n, C, 1, HW, seed=5)
    t3, s3 = torch.from_numpy(tgt).to(DEV), torch.from_numpy(src).to(DEV)
    map3 = contrast_map(t3, s3)
    mask3, stats3 = contrast_mask(map3, [2.0, 3.0, 3.0], [0, 2, 1])
    map1 = contrast_map(t3[2:3].clone(), s3[2:3].clone())
    mask1, stats1 = contrast_mask(map1, 3.0, 1)
    assert torch.equal(map1[0], map3[2]) and torch.equal(stats1[0], stats3[2]) and torch.equal(mask1[0], mask3[2])
    # the same request at an odd element offset: every pointer misaligned for the 16-byte paths
    per = n * C * HW
    tb, sb = torch.zeros(per + 8, dtype=torch.float16, device=DEV), torch.zeros(per + 8, dtype=torch.float16, device=DEV)
    tb[1:1 + per].copy_(t3[2].reshape(-1)), sb[1:1 + per].copy_(s3[2].reshape(-1))
    mb = torch.zeros(HW + 8, dtype=torch.float32, device=DEV)
    mo = contrast_map(tb[1:1 + per].view(1, n, C, 1, HW), sb[1:1 + per].view(1, n, C, 1, HW), out=mb[1:1 + HW].view(1, 1, HW))
    assert mo.data_ptr() % 16 != 0 and torch.equal(mo[0], map3[2])
    masko, statso = contrast_mask(mo, 3.0, 1)
    assert torch.equal(masko[0], mask3[2]) and torch.equal(statso[0], stats3[2]) and mb[0] == 0 and not mb[1 + HW:].any()


@pytest.mark.parametrize("box", [(5, 9, 4, 11), (0, 3, 12, 16), (13, 16, 0, 2)])          # (y0, y1, x0, x1): inside, touching the top right, the bottom left corner
@pytest.mark.parametrize("d", [0, 1, 3])
def test_a_rectangle_of_difference_grows_by_d(box, d):
    y0, y1, x0, x1 = box
    h = w = 16
    g = np.random.default_rng(3)
    src = g.standard_normal((1, 2, 4, h, w)).astype(np.float16)
    tgt = src.copy()
    tgt[..., y0:y1, x0:x1] += np.float16(1.0)
    want = np.zeros((h, w), np.float16)
    want[max(y0 - d, 0):min(y1 + d, h), max(x0 - d, 0):min(x1 + d, w)] = 1
    _, stats, mask = _run(tgt, src, 3.0, d)
    assert stats[0, 0] > 0 and np.array_equal(mask[0, 0], want)


def test_refusals_come_before_any_launch():
    from instructany2pix_amd import _ffi
    import ctypes as C
    L, s, p = _ffi.lib(), _ffi.current_stream(), _ffi.ptr
    INVALID, SHAPE = 1, 2
    t = torch.ones(2, 2, 4, 8, 8, dtype=torch.float16, device=DEV)
    src = torch.zeros_like(t)
    cmap = torch.full((2, 8, 8), 7.0, dtype=torch.float32, device=DEV)
    mask, stats = torch.full((2, 1, 8, 8), 5.0, dtype=torch.float16, device=DEV), torch.full((2, 2), 9.0, dtype=torch.float32, device=DEV)
    fl, it = lambda *v: (C.c_float * len(v))(*v), lambda *v: (C.c_int * len(v))(*v)
    good = [p(t), p(src), p(cmap)]
    for i in range(3):
        a = list(good)
        a[i] = None
        assert L.ia2p_eps_contrast_map(s, *a, 2, 2, 4, 64) == INVALID, i
    off = lambda x, k: C.c_void_p(x.data_ptr() + k)
    assert L.ia2p_eps_contrast_map(s, off(t, 1), p(src), p(cmap), 2, 2, 4, 64) == INVALID          # misaligned for fp16
    assert L.ia2p_eps_contrast_map(s, p(t), p(src), off(cmap, 2), 2, 2, 4, 64) == INVALID          # misaligned for fp32
    for B, n, Cc, HW in ((0, 2, 4, 64), (2, 0, 4, 64), (2, 2, 0, 64), (2, 2, 4, 0), (-1, 2, 4, 64)):
        assert L.ia2p_eps_contrast_map(s, *good, B, n, Cc, HW) == SHAPE, (B, n, Cc, HW)
    gm = [p(cmap), fl(3.0, 3.0), it(1, 1), p(mask), p(stats)]
    for i in range(5):
        a = list(gm)
        a[i] = None
        assert L.ia2p_contrast_mask(s, *a, 2, 8, 8) == INVALID, i
    assert L.ia2p_contrast_mask(s, off(cmap, 2), gm[1], gm[2], p(mask), p(stats), 2, 8, 8) == INVALID
    assert L.ia2p_contrast_mask(s, p(cmap), gm[1], gm[2], off(mask, 1), p(stats), 2, 8, 8) == INVALID
    for B, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert L.ia2p_contrast_mask(s, *gm, B, h, w) == SHAPE, (B, h, w)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.ia2p_contrast_mask(s, p(cmap), fl(3.0, bad), gm[2], p(mask), p(stats), 2, 8, 8) == SHAPE, bad
    for bad in (-1, 17):
        assert L.ia2p_contrast_mask(s, p(cmap), gm[1], it(1, bad), p(mask), p(stats), 2, 8, 8) == SHAPE, bad
    with pytest.raises(ValueError, match="SHAPE.*dilate\\[1\\]=17"):
        _ffi.check(L.ia2p_contrast_mask(s, p(cmap), gm[1], it(1, 17), p(mask), p(stats), 2, 8, 8))
    torch.cuda.synchronize()
    assert bool((cmap == 7.0).all()) and bool((mask == 5.0).all()) and bool((stats == 9.0).all())      # no refused call launched anything
    assert L.ia2p_eps_contrast_map(s, *good, 2, 2, 4, 64) == 0 and L.ia2p_contrast_mask(s, p(cmap), gm[1], it(1, 16), p(mask), p(stats), 2, 8, 8) == 0
    torch.cuda.synchronize()
    assert bool((cmap == 1.0).all()) and bool((mask == 0.0).all()) and stats.tolist() == [[1.0, 1.5]] * 2


# ---- the loops --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from test_edit_batch_gpu import Models
    return Models()


def _cond(m, seed):
    from test_edit_batch_gpu import _cond
    return _cond(m, seed)


def _explicit(c):
    from instructany2pix_amd.pipeline import EMBED_KEYS, fuse_instruction_embedding
    la = fuse_instruction_embedding(c["base_embed"], c["image_embeds"], c["y"], [0.0, 0.4, 1.0], 20.0).reshape(1, -1)[0]
    return la, {k: c[k] for k in EMBED_KEYS}


def _f16(t):
    return t.to(DEV, torch.float16)


def _by_hand(pipe, conds, steps, scales, knobs, noises, max_rows):
    """the estimate of a group from the launches themselves: add_noise, the two UNet evaluations in chunks, the two mask launches"""
    from instructany2pix_amd.auto_mask import contrast_map, contrast_mask
    from instructany2pix_amd.ddim import conditioning, get_add_time_ids
    from instructany2pix_amd.scheduler import DDIMScheduler, fused_update_v, kept_steps
    unet = pipe.pipe.unet
    ns = [k["num_maps"] for k in knobs]
    ts = []
    for n_steps, k in zip(steps, knobs):
        sch = DDIMScheduler.from_config(pipe.pipe.scheduler.config)
        sch.set_timesteps(n_steps)
        ts.append(int(sch.timesteps[kept_steps(n_steps, k["strength"])[0]]))
    rep = lambda xs: torch.cat([_f16(x).expand(n, *x.shape[1:]) for x, n in zip(xs, ns)]).contiguous()
    x0, z = rep([c["base_latents"] for c in conds]), torch.cat([_f16(zz) for zz in noises]).contiguous()
    coef = torch.tensor([(1.0,) + tuple(sch.add_noise_coeffs(t)) for t, n in zip(ts, ns) for _ in range(n)], dtype=torch.float32, device=DEV)
    x = fused_update_v(x0, z, None, coef, torch.empty_like(x0))
    t_rows = torch.tensor([float(t) for t, n in zip(ts, ns) for _ in range(n)])
    sc_rows = torch.tensor([float(s) for s, n in zip(scales, ns) for _ in range(n)])
    ip, _ = pipe.ip_adapter_xl.get_image_embeds(clip_image_embeds=torch.stack([_explicit(c)[0] for c in conds]), mode="global")
    src_ctx, src_pool = rep([c["negative_prompt_embeds"] for c in conds]), rep([c["negative_pooled_prompt_embeds"] for c in conds])
    tgt_ctx = rep([torch.cat([_f16(c["prompt_embeds"]), ip[i:i + 1]], dim=1) for i, c in enumerate(conds)])
    tgt_pool = rep([c["pooled_prompt_embeds"] for c in conds])
    tid = get_add_time_ids(unet, (128, 128), (0, 0), (128, 128), int(src_pool.shape[-1]))
    eps_src, eps_tgt = torch.empty_like(x), torch.empty_like(x)
    for lo in range(0, x.shape[0], max_rows):
        hi = min(lo + max_rows, x.shape[0])
        ctx, added = conditioning(DEV, src_ctx[lo:hi], src_pool[lo:hi], tid)
        unet(x[lo:hi], t_rows[lo:hi], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps_src[lo:hi])
    for lo in range(0, x.shape[0], max_rows):
        hi = min(lo + max_rows, x.shape[0])
        ctx, added = conditioning(DEV, tgt_ctx[lo:hi], tgt_pool[lo:hi], tid)
        unet(x[lo:hi], t_rows[lo:hi], encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps_tgt[lo:hi], ip_scales=sc_rows[lo:hi])
    out, s0 = [], 0
    for n, k in zip(ns, knobs):
        cmap = contrast_map(eps_tgt[s0:s0 + n][None], eps_src[s0:s0 + n][None])
        mask, stats = contrast_mask(cmap, k["ratio"], k["dilate"])
        out.append((mask, cmap, stats[0]))
        s0 += n
    return out


KNOB = dict(num_maps=3, strength=0.5, ratio=2.0, dilate=0)          # ratio 2: tau is the mean, so some cell is on and some cell is off whatever the weights


def _noise(seed, n):
    return torch.randn(n, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()


def test_the_estimate_is_its_stages_by_hand_and_denoise_under_it_is_denoise_under_that_mask(models):
    pipe = models.pipeline()
    c = _cond(models, 300)
    la, emb = _explicit(c)
    z = _noise(1, 3)
    mask, cmap, stats = pipe.estimate_edit_mask(c["base_latents"], la, **emb, num_inference_steps=4, scale=0.8, auto_mask=dict(KNOB, noise=z))
    (hm, hc, hs), = _by_hand(pipe, [c], [4], [0.8], [KNOB], [z], 3)
    assert torch.equal(mask, hm) and torch.equal(cmap, hc) and torch.equal(stats, hs)
    assert tuple(mask.shape) == (1, 1, 16, 16) and mask.dtype == torch.float16 and 0 < float(mask.float().mean()) < 1
    assert tuple(cmap.shape) == (1, 16, 16) and cmap.dtype == torch.float32 and float(stats[1]) == float(stats[0])      # ratio 2: tau = mean
    two = pipe.estimate_edit_mask(c["base_latents"], la, **emb, num_inference_steps=4, scale=0.8, auto_mask=dict(KNOB, noise=z, max_rows=2))
    (hm2, hc2, _), = _by_hand(pipe, [c], [4], [0.8], [KNOB], [z], 2)                 # rows in chunks of at most max_rows
    assert torch.equal(two[0], hm2) and torch.equal(two[1], hc2)
    # denoise
    kw = dict(**emb, num_inference_steps=4, cfg=4.0, scale=0.8, noise=c["polar_noise"])
    base = _f16(c["base_latents"])
    reset = lambda: pipe.ip_adapter_xl.set_scale(1.0)           # (the inversion, and eps_src with it, runs under the scale the last sampling left on the processors)
    reset()
    auto, inv = pipe.denoise(c["base_latents"], la, **kw, auto_mask=dict(KNOB, noise=z))
    reset()
    given, inv_g = pipe.denoise(c["base_latents"], la, **kw, edit_mask=mask)
    assert torch.equal(auto, given) and torch.equal(inv, inv_g)
    inside = (mask != 0).expand(1, 4, 16, 16)
    assert torch.equal(auto[~inside], base[~inside]) and not torch.equal(auto[inside], base[inside])
    # with a user mask too: the product of the two latent masks
    user = torch.zeros(1, 1, 16, 16)
    user[..., :8] = 1
    reset()
    both, _ = pipe.denoise(c["base_latents"], la, **kw, auto_mask=dict(KNOB, noise=z), edit_mask=user)
    reset()
    prod, _ = pipe.denoise(c["base_latents"], la, **kw, edit_mask=mask * user.to(DEV))
    assert torch.equal(both, prod) and 0 < float((mask * user.to(DEV)).sum()) < float(mask.sum())
    pipe.ip_adapter_xl.set_scale(1.0)


def test_a_seeded_request_draws_the_same_estimate_noise_alone_and_in_a_batch(models):
    from instructany2pix_amd import noise
    from instructany2pix_amd.batch import EditRequest
    from instructany2pix_amd.auto_mask import estimate_requests
    pipe = models.pipeline()
    cs = [_cond(models, 310 + i) for i in range(2)]
    knob = dict(KNOB, num_maps=2)
    z = noise.randn_seeded([77], noise.DRAW_AUTO_MASK, (2 * 4 * 16 * 16,), torch.float16, DEV).view(2, 4, 16, 16)      # element k per + e: noise k, element e
    la, emb = _explicit(cs[0])
    seeded = pipe.estimate_edit_mask(cs[0]["base_latents"], la, **emb, num_inference_steps=3, seed=77, auto_mask=knob)
    supplied = pipe.estimate_edit_mask(cs[0]["base_latents"], la, **emb, num_inference_steps=3, auto_mask=dict(knob, noise=z.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(seeded, supplied))
    state = torch.get_rng_state()
    reqs = [EditRequest(base_latents=c["base_latents"], latent_la=_explicit(c)[0], **_explicit(c)[1], num_inference_steps=3, seed=s, auto_mask=knob)
            for c, s in zip(cs[::-1], (5, 77))]                                      # the same request as row 1 of a group of two
    est = estimate_requests(pipe, reqs, group=2)
    (_, hand), = [_by_hand(pipe, cs[::-1], [3, 3], [1.0, 1.0], [knob, knob], [noise.randn_seeded([5], noise.DRAW_AUTO_MASK, (2048,), torch.float16, DEV).view(2, 4, 16, 16), z], 4)]
    assert torch.equal(est[1].mask, hand[0]) and torch.equal(est[1].map, hand[1]) and torch.equal(torch.get_rng_state(), state)      # seeded: nothing from the global generator


def test_edit_batch_group_of_three_with_two_auto_masks(models):
    conds = {f"edit {i}": _cond(models, 320 + i) for i in range(3)}
    pipe = models.pipeline(conds, refiner_handoff="latent")
    cs, steps = list(conds.values()), [3, 5, 4]
    zs = [_noise(2, 2), None, _noise(3, 3)]
    knobs = [dict(num_maps=2, strength=0.5, ratio=2.0, dilate=0), None, dict(num_maps=3, strength=1.0, ratio=2.0, dilate=1)]
    autos = [None if k is None else dict(k, noise=z) for k, z in zip(knobs, zs)]
    kw = dict(num_inference_steps=steps, cfg=[4.0, 5.0, 6.0], refinement=[0.1, 0.1, 0.0], group=4)
    user = np.zeros((128, 128), np.uint8)
    user[:, :60] = 255                                                               # request 2 also carries a user mask: latent cells 0 .. 7
    got = pipe.edit_batch(list(conds), [[]] * 3, **kw, auto_masks=autos, edit_masks=[None, None, user], debug=True)
    hand = _by_hand(pipe, [cs[0], cs[2]], [3, 4], [1.0, 1.0], [knobs[0], knobs[2]], [zs[0], zs[2]], 8)
    lat_user = torch.zeros(1, 1, 16, 16, device=DEV, dtype=torch.float16)
    lat_user[..., :8] = 1
    masks = [hand[0][0], None, hand[1][0] * lat_user]
    for i, h in ((0, hand[0]), (2, hand[1])):
        msg = got[i][2]
        assert torch.equal(msg["edit_mask"], masks[i]) and torch.equal(msg["edit_mask_latent"], masks[i])
        assert torch.equal(msg["auto_mask_map"], h[1]) and torch.equal(msg["auto_mask_stats"], h[2])
        assert 0 < float(masks[i].float().mean()) < 1
    assert "edit_mask" not in got[1][2] and "auto_mask_map" not in got[1][2]
    given = pipe.edit_batch(list(conds), [[]] * 3, **kw, edit_masks=masks)           # the same masks handed in: the existing path, bit for bit
    plain = pipe.edit_batch(list(conds), [[]] * 3, **kw)
    for i in range(3):
        assert torch.equal(got[i][0], given[i][0]) and torch.equal(got[i][1], given[i][1]), i
    assert torch.equal(got[1][0], plain[1][0]) and torch.equal(got[1][1], plain[1][1])      # the request without a mask: its bits in the group with no mask anywhere
    for i in (0, 2):
        ins = (masks[i] != 0).expand(1, 4, 16, 16)
        b = _f16(cs[i]["base_latents"])
        assert torch.equal(got[i][0][~ins], b[~ins]) and torch.equal(got[i][1][~ins], b[~ins]) and not torch.equal(got[i][0][ins], b[ins])


def test_call_with_auto_mask_pil_output_and_none_changes_nothing(models):
    """tiny VAE (factor 4: 64 x 64 images over 16 x 16 latents)"""
    conds = {f"edit {i}": _cond(models, 330 + i) for i in range(2)}
    pipe = models.pipeline(conds, vae=models.vae)
    post = lambda lat: np.asarray(pipe.pipe.image_processor.postprocess(models.vae.decode_from_latents(_f16(lat)), output_type="pil")[0])
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=0.1, seed=9)
    knob = dict(KNOB, num_maps=2)
    lat = pipe("edit 0", [], **kw, auto_mask=knob, debug=True)
    m = lat[2]["edit_mask"]
    assert 0 < float(m.float().mean()) < 1 and torch.equal(m, lat[2]["edit_mask_latent"])
    again = pipe("edit 0", [], **kw, edit_mask=m)                                    # seeded: the same mask handed in gives the same latents
    assert torch.equal(lat[0], again[0]) and torch.equal(lat[1], again[1])
    ins = (m != 0).expand(1, 4, 16, 16)
    base = _f16(conds["edit 0"]["base_latents"])
    assert torch.equal(lat[0][~ins], base[~ins]) and torch.equal(lat[1][~ins], base[~ins])
    pil = pipe("edit 0", [], **kw, auto_mask=knob, edit_feather=3, output_type="pil")
    base_img = post(conds["edit 0"]["base_latents"])
    px = m[0, 0].repeat_interleave(4, 0).repeat_interleave(4, 1).cpu().numpy() != 0
    for img in (pil[0][0], pil[1][0]):
        a = np.asarray(img)
        assert np.array_equal(a[~px], base_img[~px]) and not np.array_equal(a[px], base_img[px])      # every byte outside the mask: the base image's
    with pytest.raises(ValueError, match='must be "pil" or "latent"'):
        pipe("edit 0", [], **kw, auto_mask=knob, output_type="np")
    # an unseeded request: the estimate's draw comes before the polar-mixing draw
    torch.manual_seed(4)
    un = pipe("edit 1", [], num_inference_steps=3, cfg=4.0, refinement=0.0, auto_mask=knob, debug=True)
    torch.manual_seed(4)
    z = torch.randn(2, 4, 16, 16, dtype=torch.float16)
    la, emb = _explicit(conds["edit 1"])
    want = pipe.estimate_edit_mask(conds["edit 1"]["base_latents"], la, **emb, num_inference_steps=3, auto_mask=dict(knob, noise=z))
    assert torch.equal(un[2]["edit_mask"], want[0]) and torch.equal(un[2]["auto_mask_map"], want[1])
    # auto_mask=None: the bits and the global RNG state of the call without the keyword
    insts = list(conds)
    outs, states = [], []
    for extra, bextra in (({}, {}), (dict(auto_mask=None), dict(auto_masks=None))):
        torch.manual_seed(6)
        one = pipe("edit 0", [], num_inference_steps=3, cfg=4.0, refinement=0.1, **extra)
        many = pipe.edit_batch(insts, [[], []], num_inference_steps=3, cfg=4.0, refinement=0.1, group=2, **bextra)
        outs.append([one[0], one[1]] + [t for r in many for t in r[:2]])
        states.append(torch.get_rng_state())
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and torch.equal(*states)
