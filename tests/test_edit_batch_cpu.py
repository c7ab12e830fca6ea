"""Host side of batched whole-request serving (instructany2pix_amd/batch.py: `refine_tables`, `inpaint_tables`, argument handling of `refine_batch` /
`inpaint_batch` / `edit_batch`). Needs no GPU: the tables of the joint loops are pure host arithmetic and every refusal comes before the first launch.

What must hold: row r of a group's `[iterations][requests]` tables carries exactly what the scheduler gives request r alone on the serial pipelines'
path (img2img.py / inpaint.py: the `get_timesteps` tail, the start coefficients, the per-step coefficients), and a request that is through is HELD:
evaluated at its last timestep, moved with (g, 1, 0), blended with (1, 0)."""
from types import SimpleNamespace

import pytest
import torch

N_STEPS, STRENGTHS, KEPT = 8, (0.3, 0.5, 1.0), (2, 4, 8)        # int(8 * s) steps: rows of 2, 4 and 8 steps


def test_refine_tables_equal_the_euler_scheduler_per_request():
    from instructany2pix_amd.batch import refine_tables
    from instructany2pix_amd.scheduler import EulerDiscreteScheduler
    cfg = EulerDiscreteScheduler().config
    tb = refine_tables(cfg, STRENGTHS, N_STEPS, 5.0)
    assert tb.steps == list(KEPT) and len(tb.timesteps) == len(tb.input_scale) == len(tb.coef) == 8
    for r, n in enumerate(KEPT):
        sch = EulerDiscreteScheduler.from_config(cfg)            # the request alone
        sch.set_timesteps(N_STEPS)
        t_start = N_STEPS - n
        tail = sch.timesteps[t_start:]
        assert len(tail) == n
        assert tb.start_sigma[r] == float(sch.sigmas[sch.index_for_timestep(tail[0])]) == float(sch.sigmas[t_start])
        for k in range(8):
            if k < n:
                assert tb.timesteps[k][r] == float(tail[k])
                assert tb.input_scale[k][r] == sch.input_scale(t_start + k)
                assert tb.coef[k][r] == (5.0,) + sch.step_coeffs(t_start + k)
                assert tb.coef[k][r][1] == 1.0 and tb.coef[k][r][2] < 0
            else:                                                # held: its last timestep, latents kept
                assert tb.timesteps[k][r] == float(tail[-1]) == float(sch.timesteps[-1])
                assert tb.input_scale[k][r] == sch.input_scale(N_STEPS - 1)
                assert tb.coef[k][r] == (5.0, 1.0, 0.0)
    assert tb.coef[7][2][2] == tb.coef[1][0][2] == tb.coef[3][1][2] == -float(sch.sigmas[N_STEPS - 1])      # every request's last move lands on sigma = 0
    # a group of one short request has as many iterations as that request has steps
    one = refine_tables(cfg, [0.3], N_STEPS, 5.0)
    assert len(one.timesteps) == 2 and [row[0] for row in one.timesteps] == [row[0] for row in tb.timesteps[:2]]


def test_inpaint_tables_equal_the_ddim_scheduler_per_request():
    from instructany2pix_amd.batch import inpaint_tables
    from instructany2pix_amd.scheduler import DDIMScheduler
    cfg = DDIMScheduler().config
    tb = inpaint_tables(cfg, STRENGTHS, N_STEPS, 7.5)
    assert tb.steps == list(KEPT) and len(tb.timesteps) == len(tb.coef) == len(tb.blend) == 8
    for r, (n, s) in enumerate(zip(KEPT, STRENGTHS)):
        sch = DDIMScheduler.from_config(cfg)
        sch.set_timesteps(N_STEPS)
        tail = [int(t) for t in sch.timesteps[N_STEPS - n:]]
        if s == 1.0:                                             # x = noise * init_noise_sigma, the image latents do not enter
            assert tb.start[r] == (1.0, 0.0, 1.0)
        else:
            assert tb.start[r] == (1.0,) + sch.add_noise_coeffs(tail[0])
        for k in range(8):
            if k < n:
                assert tb.timesteps[k][r] == float(tail[k])
                assert tb.coef[k][r] == (7.5,) + sch.step_coeffs(tail[k])
                assert tb.blend[k][r] == (sch.add_noise_coeffs(tail[k + 1]) if k < n - 1 else (1.0, 0.0))      # no re-noising after the last step
            else:
                assert tb.timesteps[k][r] == float(tail[-1])
                assert tb.coef[k][r] == (7.5, 1.0, 0.0) and tb.blend[k][r] == (1.0, 0.0)
    assert tb.blend[0][0] != (1.0, 0.0) and tb.blend[1][0] == (1.0, 0.0)


def test_a_strength_that_leaves_no_step_is_refused_naming_the_request():
    from instructany2pix_amd.batch import inpaint_tables, refine_tables
    from instructany2pix_amd.scheduler import DDIMScheduler, EulerDiscreteScheduler
    for tables, cfg in ((refine_tables, EulerDiscreteScheduler().config), (inpaint_tables, DDIMScheduler().config)):
        with pytest.raises(ValueError, match=r"number of pipeline steps is 0 .*request 1"):
            tables(cfg, [0.5, 0.01, 0.5], 50, 5.0)
        with pytest.raises(ValueError, match=r"should in \[0.0, 1.0\].*request 0"):
            tables(cfg, [1.5], 50, 5.0)


def test_per_request_broadcasts_scalars_and_checks_lengths():
    from instructany2pix_amd.batch import _is_one_h, per_request
    assert per_request(0.7, 3, "alpha") == [0.7, 0.7, 0.7]
    assert per_request([1, 2, 3], 3, "cfg") == [1, 2, 3] and per_request((4.0, 5.0), 2, "cfg") == [4.0, 5.0]
    with pytest.raises(ValueError, match="`cfg` has 2 entries for 3 requests"):
        per_request([1, 2], 3, "cfg")
    # h: one triple for all (also when N = 3), or N triples
    assert per_request([0.0, 0.4, 1.0], 3, "h", _is_one_h) == [[0.0, 0.4, 1.0]] * 3
    assert per_request([[0.0, 0.4, 1.0], [1.0, 0.0, 0.5]], 2, "h", _is_one_h) == [[0.0, 0.4, 1.0], [1.0, 0.0, 0.5]]
    with pytest.raises(ValueError, match="`h` has 2 entries for 3 requests"):
        per_request([[0.0, 0.4, 1.0], [1.0, 0.0, 0.5]], 3, "h", _is_one_h)


def _refine_requests(sizes, strengths):
    from instructany2pix_amd.batch import RefineRequest
    z = torch.zeros(1, 1)
    return [RefineRequest(latents=torch.zeros(1, 4, hw, hw), prompt_embeds=z, pooled_prompt_embeds=z, negative_prompt_embeds=z,
                          negative_pooled_prompt_embeds=z, strength=s) for hw, s in zip(sizes, strengths)]


def _inpaint_requests(sizes, strengths):
    from instructany2pix_amd.batch import InpaintRequest
    z = torch.zeros(1, 1)
    return [InpaintRequest(latents=torch.zeros(1, 4, hw, hw), mask=torch.zeros(hw, hw), subject_embed=torch.zeros(4), prompt_embeds=z, pooled_prompt_embeds=z,
                           negative_prompt_embeds=z, negative_pooled_prompt_embeds=z, strength=s) for hw, s in zip(sizes, strengths)]


def test_loops_refuse_bad_arguments_before_touching_a_model():
    """the model objects are None-like stubs: a refusal that came after the first use of one would fail differently"""
    from instructany2pix_amd.batch import inpaint_batch, refine_batch
    from instructany2pix_amd.scheduler import DDIMScheduler, EulerDiscreteScheduler
    piperf = SimpleNamespace(scheduler=EulerDiscreteScheduler(), unet=None)
    ipa = SimpleNamespace(pipe=SimpleNamespace(scheduler=DDIMScheduler(), unet=None))
    for fn, model, mk in ((refine_batch, piperf, _refine_requests), (inpaint_batch, ipa, _inpaint_requests)):
        with pytest.raises(ValueError, match="share the latent size"):
            fn(model, mk([16, 24], [0.5, 0.5]))
        with pytest.raises(ValueError, match="at least one request"):
            fn(model, [])
        for group in (0, 9):
            with pytest.raises(ValueError, match=f"group={group}"):
                fn(model, mk([16], [0.5]), group=group)
        with pytest.raises(ValueError, match="NO guidance"):
            fn(model, mk([16], [0.5]), guidance_scale=1.0)
        with pytest.raises(ValueError, match=r"steps is 0 .*request 1"):
            fn(model, mk([16, 16], [0.5, 0.0]))
        with pytest.raises(ValueError, match="positive integer"):
            fn(model, mk([16], [0.5]), num_inference_steps=0)


def test_edit_batch_refuses_bad_arguments_before_any_stage():
    from instructany2pix_amd.batch import edit_batch
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    called = []
    stub = SimpleNamespace(vae=None, ip_adapter_xl=object(), piperf=None, conditioner=lambda *a, **kw: called.append(a))
    kw = dict(refinement=0.0)
    with pytest.raises(ValueError, match="2 instructions for 1 mm_data"):
        edit_batch(stub, ["a", "b"], [[]], **kw)
    with pytest.raises(ValueError, match="at least one request"):
        edit_batch(stub, [], [], **kw)
    with pytest.raises(ValueError, match="`cfg` has 3 entries for 2 requests"):
        edit_batch(stub, ["a", "b"], [[], []], cfg=[4.0, 5.0, 6.0], **kw)
    with pytest.raises(ValueError, match=r"cfg=1.0 <= 1 \(request 1\)"):
        edit_batch(stub, ["a", "b"], [[], []], cfg=[4.0, 1.0], **kw)
    for group in (0, 9):
        with pytest.raises(ValueError, match=f"group={group}"):
            edit_batch(stub, ["a"], [[]], group=group, **kw)
    with pytest.raises(ValueError, match="output_type"):
        edit_batch(stub, ["a"], [[]], output_type="jpeg", **kw)
    with pytest.raises(ValueError, match="needs the pipeline built with vae="):
        edit_batch(stub, ["a"], [[]], output_type="pil", **kw)
    with pytest.raises(ValueError, match=r"steps is 0 .*request 1"):
        edit_batch(stub, ["a", "b"], [[], []], refinement=0.0, subject_strength=[0.7, 0.01])
    with pytest.raises(ValueError, match="positive integer"):
        edit_batch(stub, ["a"], [[]], num_inference_steps=0, **kw)
    # a pipeline without a refiner: `__call__` skips the pass silently, a batch that asks for it is refused
    with pytest.raises(ValueError, match="refiner_unet="):
        edit_batch(stub, ["a", "b"], [[], []], refinement=[0.0, 0.5])
    with pytest.raises(ValueError, match="refiner_unet="):
        InstructAny2PixPipeline.edit_batch(stub, ["a"], [[]])            # the method's default refinement is 0.5, as `__call__`'s
    with pytest.raises(NotImplementedError, match="ip_ckpt"):
        edit_batch(SimpleNamespace(vae=None, ip_adapter_xl=None, piperf=None), ["a"], [[]], **kw)
    assert not called                                                    # no request was conditioned


def test_mixed_latent_sizes_are_refused_after_conditioning():
    from instructany2pix_amd.batch import edit_batch
    conds = {"a": dict(image_embeds=torch.ones(1, 8), base_embed=torch.ones(1, 8), y=torch.ones(1, 8), caption="a", base_latents=torch.zeros(1, 4, 16, 16)),
             "b": dict(image_embeds=torch.ones(1, 8), base_embed=torch.ones(1, 8), y=torch.ones(1, 8), caption="b", base_latents=torch.zeros(1, 4, 24, 24))}
    stub = SimpleNamespace(vae=None, ip_adapter_xl=object(), piperf=None, model=None, _conditions_for_batch=lambda insts, mms: [conds[i] for i in insts])
    with pytest.raises(ValueError, match="share the latent size"):
        edit_batch(stub, ["a", "b"], [[], []], refinement=0.0)


def test_the_new_symbol_is_declared_bound_and_documented():
    import os
    from instructany2pix_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "ia2p_mask_blend_v" in _ffi.SIGNATURES and len(_ffi.SIGNATURES["ia2p_mask_blend_v"][1]) == 11
    assert "ia2p_mask_blend_v(" in open(os.path.join(root, "include", "ia2p.h")).read()
    assert "ia2p_mask_blend_v" in open(os.path.join(root, "INTEGRATION.md")).read()
