"""The few-step consistency sampler on the MI355X (include/ia2p.h "Consistency sampler"; csrc/lcm.hip; scheduler.LCMScheduler; batch.lcm_sample).

  1. `ia2p_lcm_step_v` against the float64 restatement of tests/lcm_ref.py, every element within the bound counted there: guided and eps_c = NULL, rows that mix
     seeded, pointer, c_n = 0 and held, outputs in guarded buffers at a 16-byte boundary and one element past it, B = 9 across the 8-rows-by-value chunk.
  2. bit equalities: seeded launch == pointer launch fed by `randn_seeded(fp16, first)`; a row alone == the row at another place of a larger launch and at another
     alignment; out2 == out; a held row == x; a c_n = 0 row does not read `noise`.
  3. every refusal returns its status and launches nothing.
  4. the loops on the tiny configs of test_edit_batch_gpu.py, 16 x 16 latents, 3 inversion steps, LCM schedules of (3, 2, 3, 1) steps in one group."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lcm_ref as R  # noqa: E402
from test_edit_batch_gpu import Models, _cond, _traj  # noqa: E402
from unet_ops_ref import accept  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, PAD = -77.0, 96
WORST = {}


def _at(t, off):
    """a contiguous device copy of fp16 `t` that starts `off` elements past a 16-byte boundary, with sentinels around it -> (whole buffer, view)"""
    n = t.numel()
    buf = torch.full((n + PAD + 8,), SENTINEL, dtype=torch.float16, device=DEV)
    view = buf[8 + off:8 + off + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (2 * off) % 16
    return buf, view


def _untouched(buf, off, n):
    return bool((buf[:8 + off] == SENTINEL).all()) and bool((buf[8 + off + n:] == SENTINEL).all())


def _rows(case, shift, first):
    """row b is seeded / pointer / c_n = 0 / held by (b + shift) % 4 -> (coef fp32 [B, 4], firsts [B])"""
    coef, firsts = case["coef"].clone(), []
    for b in range(case["B"]):
        kind = (b + shift) % 4
        if kind == 2:
            coef[b, 3] = 0.0
        elif kind == 3:
            coef[b] = torch.tensor(R.HELD)
        firsts.append(first if kind == 0 else -1)
    return coef, firsts


def _launch(case, coef, firsts, guided, off=0, noise=None, rows=None):
    """one launch on device copies at alignment `off` -> (out, out2) on the CPU; the guard elements around both outputs must be untouched"""
    from instructany2pix_amd.scheduler import lcm_update_v
    sel = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
    x, eu, ec, nz = (_at(sel(case[k] if k != "noise" or noise is None else noise), off)[1] for k in ("x", "eu", "ec", "noise"))
    ob, out = _at(torch.zeros_like(x), off)
    ob2, out2 = _at(torch.zeros_like(x), off)
    seeds = case["seeds"] if rows is None else [case["seeds"][r] for r in rows]
    given = firsts is not None
    lcm_update_v(x, eu, ec if guided else None, sel(coef).to(DEV), out, out2, noise=nz, seeds=seeds if given else None, draws=[R.DRAW_LCM] * len(seeds) if given else None,
                 firsts=firsts)
    torch.cuda.synchronize()
    assert _untouched(ob, off, x.numel()) and _untouched(ob2, off, x.numel()), "the launch wrote outside its rows"
    return out.cpu(), out2.cpu()


# ---- 1. against fp64 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", (True, False))
@pytest.mark.parametrize("first", R.FIRSTS)
@pytest.mark.parametrize("B,per", R.KERNEL_SHAPES)
def test_the_step_meets_its_counted_bound(B, per, first, guided):
    case = R.lcm_case(B, per)
    for off in (0, 1):                                                      # at a 16-byte boundary (vector accesses), one element past it (guarded scalar ones)
        coef, firsts = _rows(case, off, first)
        out, out2 = _launch(case, coef, firsts, guided, off)
        ref, bound = R.step_ref(case, coef, *R.row_noise(case, firsts), guided=guided)
        worst = accept(f"lcm_step_v B={B} per={per} first={first} guided={guided} off={off}", out, ref, bound, axes=("b", "i"))
        assert torch.equal(out2, out)
        key = "guided" if guided else "unguided"
        WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"lcm_step_v worst max(err / bound) so far: {WORST}")


# ---- 2. bit equalities -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,per", ((3, 7), (9, 1025), (3, 4 * 16 * 16)))
def test_a_seeded_launch_is_the_pointer_launch_fed_by_randn_seeded(B, per):
    from instructany2pix_amd.noise import randn_seeded
    case = R.lcm_case(B, per)
    for first in R.FIRSTS:
        z = randn_seeded(case["seeds"], R.DRAW_LCM, (per,), torch.float16, DEV, first=first).cpu()
        seeded, _ = _launch(case, case["coef"], [first] * B, True)
        by_pointer, _ = _launch(case, case["coef"], None, True, noise=z)
        assert torch.equal(seeded, by_pointer), (B, per, first)
        assert not torch.equal(seeded, _launch(case, case["coef"], [first + 4] * B, True)[0])          # (the noise is in the result)


def test_a_row_does_not_depend_on_its_place_its_alignment_or_the_launch():
    case = R.lcm_case(9, 1025)
    coef, firsts = _rows(case, 0, 1028)
    full, full2 = _launch(case, coef, firsts, True)
    assert torch.equal(full2, full)
    for r in (0, 1, 4, 8):                                                  # alone (B = 1), at the other alignment: the row's own bits
        for off in (0, 1):
            alone, _ = _launch(case, coef, [firsts[r]], True, off, rows=[r])
            assert torch.equal(alone[0], full[r]), (r, off)
    moved, _ = _launch(case, coef, [firsts[8], firsts[3], firsts[0]], True, 1, rows=[8, 3, 0])      # three rows of it in another order: other places, another chunk
    assert torch.equal(moved[0], full[8]) and torch.equal(moved[1], full[3]) and torch.equal(moved[2], full[0])
    assert torch.equal(full[3], case["x"][3]) and torch.equal(full[7], case["x"][7])                 # held rows return x
    poisoned = case["noise"].clone()
    poisoned[2] = float("nan")                                              # row 2 carries c_n = 0 and reads its noise by pointer: it must not touch it
    again, _ = _launch(case, coef, firsts, True, noise=poisoned)
    assert torch.equal(again, full)
    unguided, _ = _launch(case, coef, firsts, False)
    assert torch.equal(unguided[3], case["x"][3]) and not torch.equal(unguided[0], full[0])


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_launch_nothing():
    from instructany2pix_amd import _ffi
    L, s, p = _ffi.lib(), _ffi.current_stream(), _ffi.ptr
    B, per = 2, 64
    x = torch.zeros(B, per, dtype=torch.float16, device=DEV)
    coef, out = torch.ones(B, 4, device=DEV), torch.full_like(x, 5.0)
    u64, u32, i64 = (lambda *v: (C.c_uint64 * len(v))(*v)), (lambda *v: (C.c_uint32 * len(v))(*v)), (lambda *v: (C.c_int64 * len(v))(*v))      # noqa: E731
    host = (u64(1, 2), u32(R.DRAW_LCM, R.DRAW_LCM), i64(0, 0))
    call = lambda x_=p(x), eu=p(x), ec=p(x), cf=p(coef), nz=p(x), h=host, o=p(out), o2=None, B_=B, per_=per: L.ia2p_lcm_step_v(s, x_, eu, ec, cf, nz, *h, o, o2, B_, per_)      # noqa: E731
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)      # noqa: E731
    INVALID, SHAPE = 1, 2
    assert call(x_=None) == INVALID and call(eu=None) == INVALID and call(cf=None) == INVALID and call(o=None) == INVALID
    for kw in (dict(x_=off(x, 1)), dict(eu=off(x, 1)), dict(ec=off(x, 1)), dict(nz=off(x, 1)), dict(o=off(out, 1)), dict(o2=off(out, 1)), dict(cf=off(coef, 2))):
        assert call(**kw) == INVALID, kw
    assert call(nz=None, h=(None, None, None)) == INVALID                   # nobody seeded and no noise
    assert call(nz=None, h=(host[0], host[1], i64(0, -1))) == INVALID       # row 1 is not seeded
    for h in ((host[0], None, None), (None, host[1], host[2]), (host[0], host[1], None)):
        assert call(h=h) == INVALID, h                                      # the three host arrays come together
    assert call(B_=0) == SHAPE and call(B_=-1) == SHAPE and call(per_=0) == SHAPE
    assert call(h=(host[0], host[1], i64(0, 2))) == SHAPE                   # not a multiple of 4
    assert call(h=(host[0], host[1], i64(2 ** 34 - 60, 0))) == SHAPE        # 2^34 - 60 + 64 > 2^34
    assert call(h=(host[0], host[1], i64(2 ** 34, 0))) == SHAPE
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(call(per_=0))
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())                                         # no refused call launched anything
    assert call(nz=None) == 0 and call(ec=None, h=(None, None, None)) == 0 and call(h=(host[0], host[1], i64(2 ** 34 - 64, -5))) == 0
    torch.cuda.synchronize()
    assert not bool((out == 5.0).any())


# ---- 4. the loops ---------------------------------------------------------------------------------------------------------------------------------------------------
LCM_STEPS = (3, 2, 3, 1)
KW = dict(num_inference_steps=3, cfg=4.0, refinement=0.0, subject_strength=0.0)


@pytest.fixture(scope="module")
def models():
    return Models()


def _request(c, **kw):
    from instructany2pix_amd.batch import EditRequest
    from instructany2pix_amd.pipeline import embeds
    kw.setdefault("sampler", "lcm")
    return EditRequest(base_latents=c["base_latents"], latent_la=c["image_embeds"].reshape(-1), **embeds(c), num_inference_steps=3, cfg=kw.pop("cfg", 4.0), **kw)


def test_sample_batch_under_lcm_is_the_loop_written_by_hand(models):
    """the same `unet` and `lcm_update_v` launches, the tables built from tests/lcm_ref.py: bit for bit. Rows: seeded, supplied noise, seeded, seeded (one step)"""
    from instructany2pix_amd.batch import sample_batch
    from instructany2pix_amd.ddim import conditioning, get_add_time_ids
    from instructany2pix_amd.scheduler import DDIMScheduler, lcm_update_v
    pipe = models.pipeline()
    unet, cfgs, n, g = pipe.pipe.unet, DDIMScheduler().config, 4, (4.0, 7.5, 3.0, 5.0)
    cs = [_cond(models, 500 + i) for i in range(n)]
    cat = lambda k: torch.cat([c[k] for c in cs]).to(DEV)      # noqa: E731
    ip, ip_un = pipe.ip_adapter_xl.get_image_embeds(clip_image_embeds=torch.stack([c["image_embeds"].reshape(-1) for c in cs]), mode="global")
    cond_ctx, uncond_ctx = torch.cat([cat("prompt_embeds"), ip], dim=1), torch.cat([cat("negative_prompt_embeds"), ip_un], dim=1)
    x = cat("polar_noise")
    seeds, scales = [21, None, 23, 24], [1.0, 0.5, 0.8, 1.0]
    noise1 = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3)).half()
    got = sample_batch(unet, cfgs, x, cond_ctx, uncond_ctx, cat("pooled_prompt_embeds"), cat("negative_pooled_prompt_embeds"), LCM_STEPS, g, scales, sampler="lcm",
                       step_noise=[None, noise1, None, None], seeds=seeds)
    # by hand
    per = x[0].numel()
    ctx, added = conditioning(DEV, cond_ctx, cat("pooled_prompt_embeds"), get_add_time_ids(unet, (128, 128), (0, 0), (128, 128), cs[0]["pooled_prompt_embeds"].shape[-1]),
                              uncond_ctx, cat("negative_pooled_prompt_embeds"))
    sc = torch.tensor(scales * 2, dtype=torch.float32).to(DEV)
    model_in = torch.cat([x, x]).contiguous()
    eps, nxt = torch.empty_like(model_in), torch.empty_like(model_in)
    for i in range(3):
        live = [i < m for m in LCM_STEPS]
        ts = [float(R.timesteps(m)[min(i, m - 1)]) for m in LCM_STEPS]
        coef = [((g[r],) + R.step_coeffs(m, i)) if live[r] else R.HELD for r, m in enumerate(LCM_STEPS)]
        firsts = [R.first_of(i, per) if live[r] and seeds[r] is not None else -1 for r in range(n)]
        z = torch.zeros_like(x)
        if i == 0:
            z[1] = noise1[0].to(DEV)
        unet(model_in, torch.tensor(ts + ts, dtype=torch.float32).to(DEV), encoder_hidden_states=ctx, added_cond_kwargs=added, out=eps, ip_scales=sc)
        lcm_update_v(model_in[:n], eps[:n], eps[n:], torch.tensor(coef, dtype=torch.float32).to(DEV), nxt[:n], nxt[n:], noise=z,
                     seeds=[0 if s is None else s for s in seeds], draws=[R.DRAW_LCM] * n, firsts=firsts)
        model_in, nxt = nxt, model_in
    assert torch.equal(got, model_in[:n])
    assert bool(torch.isfinite(got).all()) and not torch.equal(got[0], x[0])


def test_scheduler_step_is_the_launch_with_the_noise_it_draws():
    """`LCMScheduler.step` draws fp16 normals of the output's shape from the CPU generator and goes through the pointer path: within the kernel's bound of fp64"""
    from instructany2pix_amd.scheduler import LCMScheduler
    case = R.lcm_case(2, 4 * 16 * 16)
    sch = LCMScheduler()
    sch.set_timesteps(3)
    x, eps = case["x"].view(2, 4, 16, 16).to(DEV), case["eu"].view(2, 4, 16, 16).to(DEV)
    for i, t in enumerate(sch.timesteps):
        gen = torch.Generator().manual_seed(40 + i)
        got = sch.step(eps, t, x, generator=gen)[0]
        z = torch.randn(eps.shape, generator=torch.Generator().manual_seed(40 + i), dtype=torch.float16) if i < 2 else torch.zeros_like(eps).cpu()
        coef = torch.tensor([(1.0,) + R.step_coeffs(3, i)] * 2, dtype=torch.float32)
        ref, bound = R.step_ref(case, coef, z.double().view(2, -1), torch.zeros(2, 4 * 16 * 16, dtype=torch.float64), guided=False)
        accept(f"LCMScheduler.step {i}", got.cpu().view(2, -1), ref, bound)


@pytest.fixture(scope="module")
def served(models):
    """four seeded LCM requests, schedules of (3, 2, 3, 1) steps, through one `denoise_batch` group: shared by the tests below and left unchanged"""
    conds = [_cond(models, 600 + i) for i in range(8)]
    pipe = models.pipeline()
    seeds = [2000 + 13 * i for i in range(8)]
    reqs = [_request(conds[i], seed=seeds[i], sample_steps=LCM_STEPS[i]) for i in range(4)]
    out, inv = pipe.denoise_batch(reqs, group=4)
    assert bool(torch.isfinite(out).all())
    return pipe, conds, seeds, out


def test_a_seeded_request_keeps_its_bits_next_to_other_requests_and_at_another_place(served):
    pipe, conds, seeds, out = served
    order, steps = [4, 5, 0, 6], (2, 3, 3, 1)
    torch.manual_seed(2)
    moved, _ = pipe.denoise_batch([_request(conds[i], seed=seeds[i], sample_steps=m) for i, m in zip(order, steps)], group=4)
    assert torch.equal(moved[2], out[0])
    assert not torch.equal(moved[0], out[1])


def test_seeded_and_unseeded_requests_share_a_group_and_a_supplied_step_noise_wins(served):
    pipe, conds, seeds, out = served
    zs = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(8)).half()
    group = lambda: [_request(conds[0], seed=seeds[0], sample_steps=3), _request(conds[1], noise=conds[1]["polar_noise"], sample_steps=3),      # noqa: E731
                     _request(conds[2], noise=conds[2]["polar_noise"], seed=77, step_noise=zs, sample_steps=3),
                     _request(conds[2], noise=conds[2]["polar_noise"], step_noise=zs, sample_steps=3), _request(conds[2], noise=conds[2]["polar_noise"], seed=77, sample_steps=3)]
    torch.manual_seed(5)
    a, _ = pipe.denoise_batch(group(), group=8)
    torch.manual_seed(5)
    b, _ = pipe.denoise_batch(group(), group=8)
    torch.manual_seed(6)
    c, _ = pipe.denoise_batch(group(), group=8)
    assert torch.equal(a, b)
    assert torch.equal(c[0], a[0]) and not torch.equal(c[1], a[1])          # the seeded request does not look at the global generator, the unseeded one draws from it
    assert torch.equal(c[2:], a[2:])
    assert torch.equal(a[2], a[3]) and not torch.equal(a[2], a[4])          # a supplied step noise wins over the seed


def test_call_with_the_seed_serves_its_edit_batch_row_from_the_same_draws(models, monkeypatch):
    """`__call__(sampler="lcm", seed=s)` against the request's `edit_batch` row: the bar of test_noise_gpu.py; both ask the update launch for the same stream"""
    from instructany2pix_amd import batch
    conds = {f"edit {i}": _cond(models, 700 + i) for i in range(4)}
    for c in conds.values():
        del c["polar_noise"]
    pipe = models.pipeline(conds, refiner_handoff="latent")
    insts, seeds = list(conds), [3000 + 7 * i for i in range(4)]
    asked, real = [], batch.lcm_update_v

    def spy(*a, seeds=None, draws=None, firsts=None, **kw):
        asked.append([(s, d, f) for s, d, f in zip(seeds, draws, firsts)])
        return real(*a, seeds=seeds, draws=draws, firsts=firsts, **kw)
    monkeypatch.setattr(batch, "lcm_update_v", spy)
    out = pipe.edit_batch(insts, [[]] * 4, seeds=seeds, samplers="lcm", sample_steps=3, group=4, **KW)
    in_batch, asked[:] = [row[1] for row in asked], []
    nr, oo, msg = pipe(insts[1], [], seed=seeds[1], sampler="lcm", sample_steps=3, **KW)
    monkeypatch.undo()
    rel, cos = _traj(nr, out[1][0])
    print(f"__call__(sampler='lcm', seed) vs edit_batch row: rel-L2 {rel:.3e} cos {cos:.6f}")
    assert rel < 3e-2 and cos > 0.999, (rel, cos)
    P = 4 * 16 * 16
    assert [row[0] for row in asked] == in_batch == [(seeds[1], batch._noise.DRAW_LCM, k * P) for k in range(3)]


def test_an_unguided_group_runs_the_conditional_rows_alone(models, monkeypatch):
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    conds = {f"edit {i}": _cond(models, 800 + i) for i in range(2)}
    for c in conds.values():
        del c["polar_noise"]
    pipe = models.pipeline(conds, refiner_handoff="latent")
    insts, rows, real = list(conds), [], HipUNet2DConditionModel.__call__

    def counted(self, sample, *a, **kw):
        rows.append(sample.shape[0])
        return real(self, sample, *a, **kw)
    monkeypatch.setattr(HipUNet2DConditionModel, "__call__", counted)
    kw = dict(KW, cfg=1.0)
    out = pipe.edit_batch(insts, [[]] * 2, seeds=[31, 32], samplers="lcm", sample_steps=3, group=4, **kw)
    assert rows == [2] * 6                                                  # 3 inversion evaluations and 3 sampling evaluations, B_eff = n = 2 each
    guided = pipe.edit_batch(insts, [[]] * 2, seeds=[31, 32], samplers="lcm", sample_steps=3, group=4, **KW)
    assert rows[6:] == [2] * 3 + [4] * 3 and not torch.equal(guided[0][0], out[0][0])
    monkeypatch.undo()
    nr, _, _ = pipe(insts[0], [], seed=31, sampler="lcm", sample_steps=3, **kw)
    rel, cos = _traj(nr, out[0][0])
    print(f"unguided __call__ vs edit_batch row: rel-L2 {rel:.3e} cos {cos:.6f}")
    assert rel < 3e-2 and cos > 0.999, (rel, cos)
    with pytest.raises(ValueError, match="cannot share a call"):
        pipe.edit_batch(insts, [[]] * 2, seeds=[31, 32], samplers="lcm", group=4, **dict(KW, cfg=[1.0, 4.0]))


def test_under_an_edit_mask_the_base_latents_come_back_outside_it(served):
    from instructany2pix_amd.pipeline import embeds
    pipe, conds, seeds, _ = served
    mask = torch.zeros(1, 1, 16, 16)
    mask[..., 3:11, 5:14] = 1.0
    zs = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(9)).half()
    reqs = [_request(conds[0], seed=seeds[0], sample_steps=3, edit_mask=mask), _request(conds[1], seed=seeds[1], sample_steps=2),
            _request(conds[2], noise=conds[2]["polar_noise"], step_noise=zs, sample_steps=3, edit_mask=mask)]
    out, _ = pipe.denoise_batch(reqs, group=4)
    keep = (mask[0] == 0).expand(4, 16, 16).to(DEV)
    for r in (0, 2):
        base = conds[r]["base_latents"][0].half().to(DEV)
        assert torch.equal(out[r][keep], base[keep]), r                     # bit for bit where the latent mask is 0
        assert not bool((out[r][~keep] == base[~keep]).all()) and bool(torch.isfinite(out[r]).all())
    plain, _ = pipe.denoise_batch([_request(conds[1], seed=seeds[1], sample_steps=2)], group=4)      # the request without a mask carries all ones: served as without
    rel, cos = _traj(out[1], plain[0])
    assert rel < 3e-2 and cos > 0.999, (rel, cos)
    alone, _ = pipe.denoise(conds[0]["base_latents"], conds[0]["image_embeds"].reshape(-1), **embeds(conds[0]), num_inference_steps=3, cfg=4.0, seed=seeds[0], sampler="lcm", sample_steps=3, edit_mask=mask)
    base = conds[0]["base_latents"][0].half().to(DEV)
    assert torch.equal(alone[0][keep], base[keep])
    rel, cos = _traj(alone[0], out[0])
    print(f"masked LCM, serial vs batched: rel-L2 {rel:.3e} cos {cos:.6f}")
    assert rel < 3e-2 and cos > 0.999, (rel, cos)


def test_sample_adapters_are_active_for_the_sampling_stage_only_and_leave_no_trace(models, monkeypatch):
    from instructany2pix_amd import batch
    from instructany2pix_amd.pipeline import embeds
    from test_lora_gpu import LORA_MODULES, _touched_bits, make_adapter
    conds = [_cond(models, 900 + i) for i in range(2)]
    pipe = models.pipeline()
    reqs = lambda: [_request(c, seed=50 + i, sample_steps=2) for i, c in enumerate(conds)]      # noqa: E731
    try:
        pipe.load_lora_weights(make_adapter(models.bcfg, LORA_MODULES, rank=4, seed=31), "fast", text_encoder_keys="skip")
        pipe.load_lora_weights(make_adapter(models.bcfg, LORA_MODULES[:4], rank=3, seed=33), "style", text_encoder_keys="skip")
        pipe.set_adapters(["style"], [0.7])
        state, bits = pipe.pipe.unet.active_adapters(), _touched_bits(models.base, LORA_MODULES[:5])
        same = lambda: pipe.pipe.unet.active_adapters() == state == [("style", 0.7)] and all(torch.equal(v, bits[k]) for k, v in _touched_bits(models.base, LORA_MODULES[:5]).items())      # noqa: E731
        plain, inv = pipe.denoise_batch(reqs(), group=4)
        seen, real_sample, real_invert = [], batch.sample_batch, batch.invert_batch
        monkeypatch.setattr(batch, "invert_batch", lambda *a, **kw: seen.append(("invert", pipe.get_active_adapters())) or real_invert(*a, **kw))
        monkeypatch.setattr(batch, "sample_batch", lambda *a, **kw: seen.append(("sample", pipe.pipe.unet.active_adapters())) or real_sample(*a, **kw))
        fast, inv2 = pipe.denoise_batch(reqs(), group=4, sample_adapters=(["fast", "style"], [1.0, 0.7]))
        assert seen == [("invert", ["style"]), ("sample", [("fast", 1.0), ("style", 0.7)])]
        assert same() and torch.equal(inv2, inv) and not torch.equal(fast, plain)                # the inversion ran on the weights the caller left active
        pipe.set_adapters(["fast", "style"], [1.0, 0.7])
        monkeypatch.undo()
        whole, _ = pipe.denoise_batch(reqs(), group=4)
        pipe.set_adapters(["style"], [0.7])
        assert not torch.equal(whole, fast)                                                        # (with the adapter on throughout, the inversion differs too)

        class Boom(Exception):
            pass

        def boom(*a, **kw):
            assert pipe.get_active_adapters() == ["fast"]
            raise Boom()
        monkeypatch.setattr(batch, "sample_batch", boom)
        with pytest.raises(Boom):
            pipe.denoise_batch(reqs(), group=4, sample_adapters="fast")
        monkeypatch.undo()
        assert same()
        monkeypatch.setattr(pipe.ip_adapter_xl, "generate", boom)
        with pytest.raises(Boom):
            pipe.denoise(conds[0]["base_latents"], conds[0]["image_embeds"].reshape(-1), **embeds(conds[0]), num_inference_steps=3, cfg=4.0, seed=5, sampler="lcm",
                         sample_adapters=["fast"])
        monkeypatch.undo()
        assert same()
        one, _ = pipe.denoise(conds[0]["base_latents"], conds[0]["image_embeds"].reshape(-1), **embeds(conds[0]), num_inference_steps=3, cfg=4.0, seed=50, sampler="lcm",
                              sample_steps=2, sample_adapters=(["fast", "style"], [1.0, 0.7]))
        rel, cos = _traj(one[0], fast[0])
        assert same() and rel < 3e-2 and cos > 0.999, (rel, cos)
        with pytest.raises(ValueError, match="no adapter 'nope' is loaded"):
            pipe.denoise_batch(reqs(), group=4, sample_adapters="nope")
        assert torch.equal(pipe.denoise_batch(reqs(), group=4)[0], plain)
    finally:
        pipe.unload_lora_weights()


def test_with_every_keyword_at_none_nothing_changes_and_the_new_entry_is_never_called(models, monkeypatch):
    from instructany2pix_amd import _ffi
    conds = {f"edit {i}": _cond(models, 950 + i, n_subjects=1) for i in range(2)}
    pipe = models.pipeline(conds, refiner_handoff="latent")
    insts = list(conds)
    kw = dict(num_inference_steps=3, cfg=4.0, refinement=0.1, subject_strength=0.1)
    none = dict(sampler=None, sample_steps=None, sample_adapters=None)
    L, calls = _ffi.lib(), []
    real = L.ia2p_lcm_step_v
    monkeypatch.setattr(L, "ia2p_lcm_step_v", lambda *a: calls.append(1) or real(*a))
    a = pipe(insts[0], [], seed=4, **kw)
    pipe.ip_adapter_xl.set_scale(1.0)                # the serial inpaint `generate` leaves 0.8 on the shared processors
    b = pipe(insts[0], [], seed=4, **kw, **none)
    pipe.ip_adapter_xl.set_scale(1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    torch.manual_seed(1)
    c = pipe.edit_batch(insts, [[]] * 2, group=2, **kw)
    torch.manual_seed(1)
    d = pipe.edit_batch(insts, [[]] * 2, group=2, samplers=None, sample_steps=None, sample_adapters=None, **kw)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(c, d))
    assert calls == []
    pipe(insts[0], [], seed=4, sampler="lcm", sample_steps=2, **kw)        # (the spy sees the launch when there is one)
    pipe.ip_adapter_xl.set_scale(1.0)
    assert len(calls) == 2
