"""Host side of the few-step consistency sampler: `scheduler.LCMScheduler` against the numpy restatement of its rule (lcm_ref.py) and the tables
recorded there, `batch.lcm_tables` against the scheduler per request alone (after test_joint_loops_cpu.py), the host draw order of an unseeded call, the launch
sequences recorded by stand-ins, and every refusal before the first use of a model. Needs no GPU."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lcm_ref  # noqa: E402
from test_joint_loops_cpu import HW, STEPS, RecordingUNet, _embeds, _image_tokens  # noqa: E402

LCM_STEPS = (3, 2, 3, 1)


def _lcm(n):
    from instructany2pix_amd.scheduler import DDIMScheduler, LCMScheduler
    sch = LCMScheduler.from_config(DDIMScheduler().config)          # from the DDIM / SDXL config, as a diffusers user switches samplers
    sch.set_timesteps(n)
    return sch


def test_timesteps_equal_the_table_and_the_rule():
    for n, want in lcm_ref.TIMESTEPS.items():
        assert [int(t) for t in _lcm(n).timesteps] == want == lcm_ref.timesteps(n)
    for n in range(1, 51):
        assert [int(t) for t in _lcm(n).timesteps] == lcm_ref.timesteps(n)
    sch = _lcm(4)
    assert sch.init_noise_sigma == 1.0 and sch.scale_model_input("x", 3) == "x"
    sch.set_timesteps(2, original_inference_steps=10)               # k = 100: [999, 899, ..., 99] at indices 0, 5
    assert [int(t) for t in sch.timesteps] == [999, 499] == lcm_ref.timesteps(2, 10)


def test_step_coeffs_agree_with_the_rule_to_float64_rounding():
    """both sides are about ten float64 operations on the same float32 table, none of them cancelling: 1e-13 relative is a hundred roundings"""
    for n in (1, 2, 3, 4, 5, 8, 50):
        sch = _lcm(n)
        for i in range(n):
            got, want = sch.step_coeffs(i), lcm_ref.step_coeffs(n, i)
            assert all(abs(a - b) <= 1e-13 * abs(b) for a, b in zip(got, want)), (n, i, got, want)
        assert sch.step_coeffs(n - 1)[2] == 0.0 and all(sch.step_coeffs(i)[2] > 0 for i in range(n - 1))      # no noise after the last step only
        assert sch.renoise_coeffs(n - 1) == (1.0, 0.0)
    for i, row in enumerate(lcm_ref.COEFFS_4):                      # the recorded n = 4 rows, to the digits they carry
        assert all(abs(a - b) < 5e-8 for a, b in zip(_lcm(4).step_coeffs(i), row))


def test_the_configuration_is_the_sdxl_one_or_nothing():
    from instructany2pix_amd.scheduler import DDIMScheduler, LCMScheduler
    for kw in (dict(beta_schedule="linear"), dict(prediction_type="v_prediction"), dict(clip_sample=True), dict(thresholding=True)):
        with pytest.raises(NotImplementedError):
            LCMScheduler(**kw)
    sch = _lcm(4)
    with pytest.raises(NotImplementedError, match="strength"):
        sch.set_timesteps(4, strength=0.5)
    for n in (0, 51):
        with pytest.raises(ValueError, match="num_inference_steps"):
            sch.set_timesteps(n)
    back = DDIMScheduler.from_config(sch.config)                   # the inversion's scheduler is built from pipe.scheduler.config: the same schedule as ever
    back.set_timesteps(5)
    ref = DDIMScheduler()
    ref.set_timesteps(5)
    assert back.timesteps.tolist() == ref.timesteps.tolist() and float(back.final_alpha_cumprod) == float(ref.final_alpha_cumprod)


def test_lcm_tables_equal_the_scheduler_per_request_and_hold_the_rest():
    from instructany2pix_amd.batch import lcm_blend_tables, lcm_tables
    from instructany2pix_amd.noise import lcm_first
    from instructany2pix_amd.scheduler import DDIMScheduler
    cfg, g, per = DDIMScheduler().config, (4.0, 7.5, 10.0, 2.0), 4 * 15 * 15
    seeded = (True, False, True, True)
    ts, coef, firsts = lcm_tables(cfg, LCM_STEPS, g, per, seeded)
    blend = lcm_blend_tables(cfg, LCM_STEPS)
    assert len(ts) == len(coef) == len(firsts) == len(blend) == 3 and all(len(row) == 4 for row in ts + coef + firsts + blend)
    P = 4 * 15 * 15                                                 # 900: a multiple of 4 already
    for r, n in enumerate(LCM_STEPS):
        sch = _lcm(n)
        desc = [int(t) for t in sch.timesteps]
        for k in range(3):
            if k < n:
                assert ts[k][r] == float(desc[k]) and coef[k][r] == (g[r],) + sch.step_coeffs(k)
                assert firsts[k][r] == (k * P if seeded[r] else -1) == (lcm_first(k, per) if seeded[r] else -1)
                assert blend[k][r] == sch.renoise_coeffs(k) and (blend[k][r] == (1.0, 0.0)) == (k == n - 1)
                assert blend[k][r][1] == coef[k][r][3]             # the base latents are re-noised to the level the step itself arrives at
            else:                                                   # held: the last timestep, latents kept, nothing drawn
                assert ts[k][r] == float(desc[-1]) and coef[k][r] == lcm_ref.HELD and firsts[k][r] == -1 and blend[k][r] == (1.0, 0.0)
    assert lcm_first(2, 1023) == 2048 and lcm_first(1, 1) == 4 and lcm_ref.first_of(2, 1023) == 2048      # P rounds up to whole Philox blocks
    assert lcm_tables(cfg, LCM_STEPS, g)[2] == [[-1] * 4] * 3                                              # nobody seeded: every row reads its noise by pointer


# ---- launch sequences and the draw order ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def log(monkeypatch):
    from instructany2pix_amd import batch
    events = []

    def fused_update_v(x, eps_u, eps_c, coef, out, out2=None):
        events.append(("update", x.shape[0]))
        out.zero_()
        return out

    def lcm_update_v(x, eps_u, eps_c, coef, out, out2=None, noise=None, seeds=None, draws=None, firsts=None):
        assert tuple(coef.shape) == (x.shape[0], 4) and coef.dtype == torch.float32
        events.append(("lcm", x.shape[0], eps_c is not None, None if firsts is None else tuple(firsts)))
        out.zero_()
        return out

    def mask_blend_v(x, init, noise, mask, coef, out, out2=None):
        assert tuple(coef.shape) == (x.shape[0], 2) and tuple(mask.shape) == (x.shape[0], 1, HW, HW)
        events.append(("blend", x.shape[0]))
        return out
    monkeypatch.setattr(batch, "fused_update_v", fused_update_v)
    monkeypatch.setattr(batch, "lcm_update_v", lcm_update_v)
    monkeypatch.setattr(batch, "mask_blend_v", mask_blend_v)
    return events


def _pipe(log, scheduler=None):
    from instructany2pix_amd.scheduler import DDIMScheduler
    ipa = SimpleNamespace(get_image_embeds=lambda clip_image_embeds=None, mode=None: _image_tokens(clip_image_embeds.shape[0]))
    return SimpleNamespace(ip_adapter_xl=ipa, pipe=SimpleNamespace(unet=RecordingUNet(log, 6), scheduler=scheduler or DDIMScheduler(), vae_scale_factor=8))


def _req(n=4, **kw):
    from instructany2pix_amd.batch import EditRequest
    kw.setdefault("noise", torch.ones(1, 4, HW, HW).half())
    kw.setdefault("cfg", 4.0)
    return EditRequest(base_latents=torch.zeros(1, 4, HW, HW), latent_la=torch.zeros(32), num_inference_steps=n, **_embeds(), **kw)


def test_all_defaults_launch_what_the_parent_launches(log):
    """the sequence test_joint_loops_cpu.py records for the same group: no launch of the new update, and no draw"""
    from instructany2pix_amd.batch import denoise_batch
    state = torch.get_rng_state()
    out, inv = denoise_batch(_pipe(log), [_req(n) for n in STEPS], group=4)
    assert out.shape == inv.shape == (3, 4, HW, HW)
    assert log == [("unet", 3), ("update", 3)] * 6 + [("unet", 6), ("update", 3)] * 6
    assert torch.equal(torch.get_rng_state(), state)


def test_an_lcm_group_launches_a_unet_and_one_lcm_update_per_iteration(log):
    """steps (3, 2, 3, 1) in one group: 3 iterations; the inversion is the one it always was; seeded rows carry their firsts, held and pointer rows -1"""
    from instructany2pix_amd.batch import denoise_batch
    z = lambda n: torch.ones(n - 1, 4, HW, HW).half()      # noqa: E731
    reqs = [_req(4, sampler="lcm", sample_steps=n, seed=(None if r == 1 else 10 + r), step_noise=(z(n) if r == 1 else None)) for r, n in enumerate(LCM_STEPS)]
    out, _ = denoise_batch(_pipe(log), reqs, group=4)
    P = 4 * HW * HW
    assert out.shape == (4, 4, HW, HW)
    assert log[:8] == [("unet", 4), ("update", 4)] * 4
    assert log[8:] == [("unet", 8), ("lcm", 4, True, (0, -1, 0, 0)), ("unet", 8), ("lcm", 4, True, (P, -1, P, -1)), ("unet", 8), ("lcm", 4, True, (2 * P, -1, 2 * P, -1))]
    del log[:]
    # an assigned LCMScheduler makes None mean "lcm" (4 steps); cfg <= 1 everywhere: the conditional rows alone, eps_c = NULL
    from instructany2pix_amd.scheduler import LCMScheduler
    denoise_batch(_pipe(log, LCMScheduler()), [_req(2, cfg=1.0, seed=5), _req(2, cfg=0.0, seed=6)], group=4)
    assert log[:4] == [("unet", 2), ("update", 2)] * 2
    assert log[4:] == [e for k in range(4) for e in (("unet", 2), ("lcm", 2, False, (k * P, k * P)))]


def test_an_lcm_group_under_a_mask_blends_after_every_step_and_records_no_trajectory(log, monkeypatch):
    from instructany2pix_amd import batch
    seen = {}
    real = batch.invert_batch
    monkeypatch.setattr(batch, "invert_batch", lambda *a, **kw: seen.update(kw) or real(*a, **kw))
    mask = torch.zeros(1, 1, HW, HW).half()
    mask[..., :3, :] = 1
    reqs = [_req(2, sampler="lcm", sample_steps=n, step_noise=torch.ones(n - 1, 4, HW, HW).half(), edit_mask=(mask if r == 0 else None)) for r, n in enumerate((2, 3))]
    batch.denoise_batch(_pipe(log), reqs, group=4)
    assert "return_trajectory" not in seen
    assert log[4:] == [("unet", 4), ("lcm", 2, True, None), ("blend", 2)] * 3


def test_a_call_that_mixes_samplers_runs_a_group_per_sampler_in_request_order(monkeypatch):
    """and an unseeded LCM request draws its step noise right after its own polar-mixing noise, in step order: the order serial calls draw in"""
    from instructany2pix_amd import batch
    calls = []

    def denoise_group(pipeline, reqs, noises, masks=None, lcm=None, sample_adapters=None):
        calls.append(([r.alpha for r in reqs], noises, lcm))
        rows = torch.cat([torch.full((1, 4, HW, HW), float(r.alpha)).half() for r in reqs])
        return rows, rows
    monkeypatch.setattr(batch, "_denoise_group", denoise_group)
    shape = (1, 4, HW, HW)
    given = torch.full((1,) + shape[1:], 3.0).half()
    reqs = [_req(4, noise=None, alpha=0.0, sampler="lcm", sample_steps=3), _req(4, noise=None, alpha=1.0), _req(4, noise=None, alpha=2.0, sampler="lcm", seed=9),
            _req(4, noise=None, alpha=3.0, sampler="lcm", sample_steps=1), _req(4, noise=None, alpha=4.0, sampler="lcm", sample_steps=2, step_noise=given)]
    torch.manual_seed(77)
    out, _ = batch.denoise_batch(_pipe([]), reqs, group=2)
    after = torch.randn(1)
    torch.manual_seed(77)
    draw = lambda: torch.randn(shape, dtype=torch.float16)      # noqa: E731
    p0, s00, s01, p1, p3, p4 = draw(), draw(), draw(), draw(), draw(), draw()      # request 2 is seeded: it draws nothing; request 3 takes one step: no step noise
    assert torch.equal(after, torch.randn(1))
    assert [float(v) for v in out[:, 0, 0, 0]] == [0.0, 1.0, 2.0, 3.0, 4.0]          # results back in request order
    assert [c[0] for c in calls] == [[1.0], [0.0, 2.0], [3.0, 4.0]]                  # the DDIM group, then the LCM requests two at a time
    assert calls[0][2] is None and torch.equal(calls[0][1][0], p1)
    (n0, z0), (n2, z2) = calls[1][2]
    assert (n0, n2) == (3, 4) and z2 is None and calls[1][1][1] is None and torch.equal(calls[1][1][0], p0) and torch.equal(z0, torch.cat([s00, s01]))
    (n3, z3), (n4, z4) = calls[2][2]
    assert (n3, n4) == (1, 2) and z3 is None and z4 is given and torch.equal(calls[2][1][0], p3) and torch.equal(calls[2][1][1], p4)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_the_first_use_of_a_model():
    from instructany2pix_amd.batch import denoise_batch, edit_batch, sample_batch
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    from instructany2pix_amd.scheduler import DDIMScheduler, LCMScheduler
    never = lambda *a, **kw: pytest.fail("a refusal came after a model was used")      # noqa: E731
    unet = SimpleNamespace(device="cpu", _lora=None)
    for sch in (DDIMScheduler(), LCMScheduler()):
        pipe = SimpleNamespace(ip_adapter_xl=SimpleNamespace(get_image_embeds=never), pipe=SimpleNamespace(unet=unet, scheduler=sch, vae_scale_factor=8),
                               pipe_inversion=SimpleNamespace(inverse=never), conditioner=never, _conditions_for_batch=never, vae=None, piperf=None, model=None, any2pix_lm=None)
        cases = [(dict(sampler="euler"), "sampler must be one of"), (dict(sampler="ddim", sample_steps=4), "`sample_steps` is the length of the LCM schedule"),
                 (dict(sampler="lcm", sample_steps=0), "1 .. 50"), (dict(sampler="lcm", sample_steps=51), "1 .. 50"), (dict(sampler="lcm", sample_steps=2.0), "1 .. 50")]
        for kw, msg in cases:
            with pytest.raises(ValueError, match=msg):
                denoise_batch(pipe, [_req(3), _req(3, **kw)])
            with pytest.raises(ValueError, match=msg):
                InstructAny2PixPipeline.denoise(pipe, torch.zeros(1, 4, HW, HW), torch.zeros(32), **_embeds(), **kw)
            with pytest.raises(ValueError, match=msg):
                InstructAny2PixPipeline.__call__(pipe, "a", [], **kw)
            with pytest.raises(ValueError, match=msg):
                edit_batch(pipe, ["a", "b"], [[], []], samplers=[None, kw.get("sampler")], sample_steps=[None, kw.get("sample_steps")])
        z = torch.zeros(2, 4, HW, HW).half()
        for kw, msg in [(dict(sampler="ddim", step_noise=z), "samples with DDIM"), (dict(sampler="lcm", sample_steps=4, step_noise=z), r"\[3, 4, 8, 8\]"),
                        (dict(sampler="lcm", sample_steps=3, step_noise=z.float()), r"\[2, 4, 8, 8\]")]:
            with pytest.raises(ValueError, match=msg):
                denoise_batch(pipe, [_req(3, **kw)])
            with pytest.raises(ValueError, match=msg):
                InstructAny2PixPipeline.denoise(pipe, torch.zeros(1, 4, HW, HW), torch.zeros(32), **_embeds(), **kw)
        mixed = "cfg <= 1 .* and with cfg > 1 cannot share a call"
        with pytest.raises(ValueError, match=mixed):
            denoise_batch(pipe, [_req(3, sampler="lcm", cfg=1.0), _req(3, sampler="lcm", cfg=4.0)])
        with pytest.raises(ValueError, match=mixed):
            edit_batch(pipe, ["a", "b"], [[], []], samplers="lcm", cfg=[1.0, 4.0])
        with pytest.raises(ValueError, match="no adapter 'fast' is loaded"):
            denoise_batch(pipe, [_req(3)], sample_adapters="fast")
        with pytest.raises(ValueError, match="no adapter 'fast' is loaded"):
            InstructAny2PixPipeline.__call__(pipe, "a", [], sample_adapters=(["fast"], [0.5]))
        with pytest.raises(ValueError, match="no adapter 'fast' is loaded"):
            edit_batch(pipe, ["a"], [[]], sample_adapters=["fast"])
    # the DDIM refusal of cfg <= 1 stays as it is, next to LCM requests too
    pipe.pipe.scheduler = DDIMScheduler()
    with pytest.raises(ValueError, match="cfg=1.0 <= 1 means NO guidance"):
        denoise_batch(pipe, [_req(3, cfg=1.0), _req(3, sampler="lcm", cfg=1.0)])
    with pytest.raises(ValueError, match=r"cfg=1.0 <= 1 \(request 0\) means NO guidance"):
        edit_batch(pipe, ["a", "b"], [[], []], samplers=[None, "lcm"], cfg=1.0)
    # the loop itself: a request of more than one step needs a noise or a seed; `known` is the DDIM form
    x, e, p = torch.zeros(1, 4, HW, HW).half(), torch.zeros(1, 77, 16).half(), torch.zeros(1, 8).half()
    ru = RecordingUNet([], 6)
    with pytest.raises(ValueError, match="neither `step_noise` nor a seed"):
        sample_batch(ru, DDIMScheduler().config, x, e, e, p, p, [2], [4.0], sampler="lcm")
    with pytest.raises(ValueError, match="pass `base`, not `known`"):
        sample_batch(ru, DDIMScheduler().config, x, e, e, p, p, [1], [4.0], sampler="lcm", known=x[None], edit_mask=x[:, :1])
    with pytest.raises(ValueError, match="belong to sampler='lcm'"):
        sample_batch(ru, DDIMScheduler().config, x, e, e, p, p, [2], [4.0], step_noise=[x])
    assert ru.log == []


def test_the_serial_pipeline_refuses_the_lcm_keywords_under_ddim_and_the_trajectory_under_lcm():
    from instructany2pix_amd.ddim import StableDiffusionXLPipeline
    from instructany2pix_amd.scheduler import LCMScheduler
    z = torch.zeros(1, 4, HW, HW).half()
    pipe = StableDiffusionXLPipeline(None)
    for kw in (dict(step_noise=z), dict(noise_seed=3), dict(known_latents=z)):
        with pytest.raises(ValueError, match="belong to the LCM sampler"):
            pipe(prompt_embeds=z, pooled_prompt_embeds=z, **kw)
    pipe.scheduler = LCMScheduler()
    with pytest.raises(ValueError, match="pass `known_latents`, not `known_trajectory`"):
        pipe(prompt_embeds=z, pooled_prompt_embeds=z, known_trajectory=z[None], edit_mask=z[:, :1])
    with pytest.raises(ValueError, match="`known_latents` and `edit_mask` go together"):
        pipe(prompt_embeds=z, pooled_prompt_embeds=z, known_latents=z)


def test_denoise_swaps_the_scheduler_for_the_generate_call_and_puts_it_back_also_on_a_raise():
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    from instructany2pix_amd.scheduler import DDIMScheduler, LCMScheduler
    seen = []

    class Boom(Exception):
        pass
    for raises in (False, True):
        for mine, sampler, during in ((DDIMScheduler(), "lcm", LCMScheduler), (LCMScheduler(), "ddim", DDIMScheduler), (LCMScheduler(), None, LCMScheduler), (DDIMScheduler(), None, DDIMScheduler)):
            inner = SimpleNamespace(unet=SimpleNamespace(device="cpu", _lora=None), scheduler=mine)

            def generate(**kw):
                seen.append((type(inner.scheduler), kw["num_inference_steps"], sorted(k for k in kw if k in ("noise_seed", "step_noise", "known_latents", "known_trajectory"))))
                if raises:
                    raise Boom()
                return kw["latents"]
            stub = SimpleNamespace(pipe=inner, ip_adapter_xl=SimpleNamespace(generate=generate),
                                   pipe_inversion=SimpleNamespace(inverse=lambda **kw: SimpleNamespace(images=kw["latents"].half())))
            call = lambda: InstructAny2PixPipeline.denoise(stub, torch.zeros(1, 4, HW, HW), torch.zeros(32), **_embeds(), num_inference_steps=6,      # noqa: E731
                                                           noise=torch.ones(1, 4, HW, HW).half(), seed=4, sampler=sampler)
            if raises:
                with pytest.raises(Boom):
                    call()
            else:
                call()
            assert inner.scheduler is mine
            lcm = during is LCMScheduler
            assert seen[-1] == (during, 4 if lcm else 6, ["noise_seed"] if lcm else [])
            assert isinstance(stub.pipe_inversion.scheduler, DDIMScheduler)          # the inversion keeps DDIM and `num_inference_steps`


# ---- the reference itself: a numpy model of the kernel meets the bound, mutants of it do not -----------------------------------------------------------------
def _model(case, coef, z, guided, mutant=None):
    """lcm.hip's arithmetic in numpy float32: products of two fp32 numbers are exact in float64, so a fused multiply-add is one float64 sum rounded to fp32"""
    import numpy as np
    f32 = lambda t: t.float().numpy()      # noqa: E731
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)      # noqa: E731
    g, cx, ce, cn = [f32(coef)[:, k:k + 1] for k in range(4)]
    x, eu, ec, z = f32(case["x"]), f32(case["eu"]), f32(case["ec"]), z.astype(np.float16).astype(np.float32)
    if mutant == "guidance the wrong way round":
        eu, ec = ec, eu
    e = fma(g, ec - eu, eu) if guided or mutant == "guidance in an unguided launch" else eu
    if mutant == "eps combined in fp16":
        e = e.astype(np.float16).astype(np.float32)
    o = fma(ce, e, cx * x)
    if mutant == "noise one block late":
        z = np.roll(z, -4, axis=1)
    noisy = fma(z if mutant == "noise not scaled" else cn * np.ones_like(z), z if mutant != "noise not scaled" else np.ones_like(z), o)
    return torch.from_numpy(np.where(cn != 0, noisy, o).astype(np.float16))


@pytest.mark.parametrize("guided", (True, False))
def test_a_model_of_the_kernel_meets_the_bound_and_mutants_do_not(guided):
    from unet_ops_ref import worst
    case = lcm_ref.lcm_case(9, 1025)
    coef, firsts = case["coef"].clone(), []
    for b in range(9):
        if b % 4 == 2:
            coef[b, 3] = 0.0
        elif b % 4 == 3:
            coef[b] = torch.tensor(lcm_ref.HELD)
        firsts.append(1028 if b % 4 == 0 else -1)
    z, Ez = lcm_ref.row_noise(case, firsts)
    ref, bound = lcm_ref.step_ref(case, coef, z, Ez, guided=guided)
    ok, n, _ = worst(_model(case, coef, z.numpy(), guided), ref, bound)
    assert ok and 0.5 < n <= 1.0, n                  # (the fp16 store alone brings some element close to its half ulp)
    held = _model(case, coef, z.numpy(), guided)[3]
    assert torch.equal(held, case["x"][3])
    mutants = ["noise one block late", "noise not scaled"] + (["guidance the wrong way round", "eps combined in fp16"] if guided else ["guidance in an unguided launch"])
    for m in mutants:
        ok, n, at = worst(_model(case, coef, z.numpy(), guided, m), ref, bound)
        assert not ok and n > 1.0, (m, n)
