"""Editing inside a mask, the host side: level tables, the mask-loading rule, the numpy references of tests/edit_mask_ref.py against hand cases,
the refusals, and the launch lists of the joint loops with and without masks, recorded by the stand-ins of tests/test_joint_loops_cpu.py. Needs no GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import PIL.Image
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edit_mask_ref as R                                                                     # noqa: E402
from test_joint_loops_cpu import HW, STEPS, RecordingUNet, _embeds, _image_tokens, log        # noqa: E402,F401  (`log`: the recording fixture)


# ---- level tables -------------------------------------------------------------------------------------------------------------------------------------------
def test_known_levels_uniform_and_mixed():
    from instructany2pix_amd.scheduler import known_levels, level_table
    assert known_levels([3]) == [[3], [2], [1], [0]]
    assert known_levels([4, 4]) == [[4, 4], [3, 3], [2, 2], [1, 1], [0, 0]]
    mixed = known_levels((3, 5, 4))                 # the start, then after each of 5 iterations; a request that is through is held at level 0
    assert mixed == [[3, 5, 4], [2, 4, 3], [1, 3, 2], [0, 2, 1], [0, 1, 0], [0, 0, 0]]
    assert mixed == R.known_levels_ref((3, 5, 4)) and known_levels(STEPS) == R.known_levels_ref(STEPS)
    for n in (1, 7, 25):                            # one request: level N at the start, N - 1 - i after step i, level 0 (the base latents) after the last
        t = known_levels([n])
        assert len(t) == n + 1 and [row[0] for row in t] == list(range(n, -1, -1))
    with pytest.raises(ValueError, match="at least one step"):
        known_levels([3, 0])
    with pytest.raises(ValueError, match="at least one step"):
        known_levels([])
    t = level_table(mixed, 6, "cpu")
    assert t.dtype == torch.int32 and tuple(t.shape) == (6, 3) and t.is_contiguous() and t.tolist() == mixed
    with pytest.raises(ValueError, match=r"must lie in \[0, 5\)"):
        level_table(mixed, 5, "cpu")                # the store has 5 levels, the table asks for level 5
    with pytest.raises(ValueError, match="must lie in"):
        level_table([[0, -1]], 4, "cpu")


# ---- the mask-loading rule ----------------------------------------------------------------------------------------------------------------------------------
def test_load_edit_mask_forms_binarise_alike(tmp_path):
    from instructany2pix_amd.image_processor import load_edit_mask
    codes = np.arange(64, dtype=np.uint8).reshape(8, 8) * 4 + 2          # 2 .. 254: both sides of 128
    want = np.where(codes >= 128, 255, 0).astype(np.uint8)
    assert want.min() == 0 and want.max() == 255
    got = load_edit_mask(codes, 8, 8)
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, want)
    assert np.array_equal(load_edit_mask(codes >= 128, 8, 8), want)                                        # bool
    assert np.array_equal(load_edit_mask(codes.astype(np.float32) / 255.0, 8, 8), np.where(codes / 255.0 >= 0.5, 255, 0))      # float: at 0.5
    assert np.array_equal(load_edit_mask(np.array([[0.49, 0.5], [1.0, 0.0]]), 2, 2), [[0, 255], [255, 0]])
    assert np.array_equal(load_edit_mask(PIL.Image.fromarray(codes), 8, 8), want)                         # "L"
    assert np.array_equal(load_edit_mask(PIL.Image.fromarray(codes >= 128), 8, 8), want)                  # "1" -> "L"
    rgb = PIL.Image.fromarray(np.stack([want] * 3, axis=-1))                                              # "RGB" -> "L" (grey stays grey)
    assert rgb.mode == "RGB" and np.array_equal(load_edit_mask(rgb, 8, 8), want)
    path = tmp_path / "mask.png"
    PIL.Image.fromarray(codes).save(path)
    assert np.array_equal(load_edit_mask(str(path), 8, 8), want) and np.array_equal(load_edit_mask(path, 8, 8), want)
    assert not np.array_equal(want, want.T)
    assert np.array_equal(load_edit_mask(codes[:4], 4, 8), want[:4])                                      # height x width, not a square only


def _nearest(n_out, n_in):
    """PIL's NEAREST: output sample i reads input floor((i + 0.5) * n_in / n_out)"""
    return np.floor((np.arange(n_out) + 0.5) * n_in / n_out).astype(int)


def test_load_edit_mask_file_sized_masks_follow_the_base_image_crop():
    """a 3:2 base image file (30 x 20) loaded to 8 x 8: `resize_and_crop(..., 'middle')` scales it to 12 x 8 and keeps columns 2 .. 9; the mask goes the same way,
    NEAREST, and stays registered with the image that `loas_base_img` makes of the file"""
    from instructany2pix_amd.image_processor import fit_edit_mask, load_edit_mask
    from instructany2pix_amd.pipeline import resize_and_crop
    g = np.random.default_rng(3)
    m = np.where(g.random((20, 30)) < 0.5, 255, 0).astype(np.uint8)      # [H = 20, W = 30]
    want = m[_nearest(8, 20)][:, _nearest(12, 30)][:, 2:10]
    got = load_edit_mask(m, 8, 8, file_size=(30, 20))
    assert got.shape == (8, 8) and set(np.unique(got)) <= {0, 255} and np.array_equal(got, want)
    tall = load_edit_mask(m.T.copy(), 8, 8, file_size=(20, 30))          # 2:3: fit the width, crop rows
    assert np.array_equal(tall, want.T)
    # the image path itself, run with the same resampling, cuts the same pixels (a box on .5 edges included: 9 x 8 -> columns round(0.5) = 0 .. 7)
    for w, h in ((30, 20), (20, 30), (27, 24), (16, 16)):
        a = g.integers(0, 256, (h, w), dtype=np.uint8)
        img = PIL.Image.fromarray(a)
        near = PIL.Image.Resampling.NEAREST
        ref = img
        if w != h:                                   # resize_and_crop with NEAREST in place of its default resampling
            scaled = img.resize((int(8 * w / h), 8), near) if w > h else img.resize((8, int(8 * h / w)), near)
            lo = (max(scaled.size) - 8) / 2
            ref = scaled.crop((lo, 0, lo + 8, 8)) if w > h else scaled.crop((0, lo, 8, lo + 8))
        assert np.array_equal(np.asarray(fit_edit_mask(img, 8)), np.asarray(ref.resize((8, 8), near))), (w, h)
        assert resize_and_crop(img, (8, 8)).size == (8, 8)
    # an S x S mask is used as is even when a file size is known; the file size only adds a second accepted size
    sq = np.where(g.random((8, 8)) < 0.5, 255, 0).astype(np.uint8)
    assert np.array_equal(load_edit_mask(sq, 8, 8, file_size=(30, 20)), sq)


def test_load_edit_mask_refusals_name_the_sizes():
    from instructany2pix_amd.image_processor import check_edit_feather, load_edit_mask
    m = np.zeros((10, 12), np.uint8)
    with pytest.raises(ValueError, match=r"edit_mask is 10 x 12: expected 8 x 8 .* or 20 x 30 \(the base image file\)"):
        load_edit_mask(m, 8, 8, file_size=(30, 20))
    with pytest.raises(ValueError, match=r"edit_mask is 10 x 12: expected 16 x 16 \(height x width of the base image as the pipeline holds it\)$"):
        load_edit_mask(m, 16, 16)
    with pytest.raises(ValueError, match="one \\[H, W\\] plane"):
        load_edit_mask(np.zeros((8, 8, 3), np.uint8), 8, 8)
    with pytest.raises(TypeError, match="uint8, bool or float"):
        load_edit_mask(np.zeros((8, 8), np.int32), 8, 8)
    with pytest.raises(TypeError, match="PIL image, a numpy"):
        load_edit_mask([[0, 1]], 1, 2)
    assert [check_edit_feather(r) for r in (0, 8, 64, np.int64(3))] == [0, 8, 64, 3]
    for bad in (-1, 65, 2.5, "8", None, True):
        with pytest.raises(ValueError, match="edit_feather must be an integer radius of 0 .. 64"):
            check_edit_feather(bad)


def test_resolve_edit_mask_takes_latent_masks_as_they_are():
    from instructany2pix_amd.pipeline import intersect_subject_mask, resolve_edit_mask
    pipe = SimpleNamespace(pipe=SimpleNamespace(unet=SimpleNamespace(device=torch.device("cpu")), vae_scale_factor=4))
    lat = torch.zeros(1, 4, 2, 3)
    m = torch.tensor([[[[0.0, 1.0, 0.0], [2.0, 0.0, -0.0]]]])
    px, got = resolve_edit_mask(pipe, m, lat)
    assert got.dtype == torch.float16 and got.tolist() == [[[[0, 1, 0], [1, 0, 0]]]]
    assert px.dtype == torch.uint8 and tuple(px.shape) == (1, 8, 12) and px[0, :4, 4:8].eq(255).all() and px[0, :4, :4].eq(0).all() and int(px.sum()) == 255 * 32
    with pytest.raises(ValueError, match=r"latent mask \[1, 1, 2, 3\]"):
        resolve_edit_mask(pipe, torch.zeros(1, 1, 3, 3), lat)
    # a subject mask times the edit mask: same size, another size (NEAREST), every layout `prepare_mask` takes
    sub = torch.ones(8, 12)
    assert torch.equal(intersect_subject_mask(sub, px), px[0].float() / 255)
    assert torch.equal(intersect_subject_mask((sub * 255).to(torch.uint8)[None], px), px.float() / 255)
    assert tuple(intersect_subject_mask(torch.ones(1, 1, 4, 6), px).shape) == (1, 1, 4, 6)
    assert torch.equal(intersect_subject_mask(torch.ones(4, 6), px), px[0, ::2, ::2].float() / 255)
    assert torch.equal(intersect_subject_mask(PIL.Image.fromarray(np.full((8, 12), 255, np.uint8)), px), px[0].float() / 255)


# ---- the numpy references against hand cases ----------------------------------------------------------------------------------------------------------------
def test_the_references_on_hand_cases():
    m = np.zeros((1, 4, 8), np.uint8)
    m[0, 3, 5] = 128                                # one pixel at the threshold, in block (1, 2) of f = 2 / block (0, 1) of f = 4
    m[0, 0, 0] = 127                                # below it
    assert R.mask_to_latent_ref(m, 2).tolist() == [[[[0, 0, 0, 0], [0, 0, 1, 0]]]]
    assert R.mask_to_latent_ref(m, 4).tolist() == [[[[0, 1]]]] and R.mask_to_latent_ref(m, 1)[0, 0].sum() == 1
    assert R.mask_to_latent_ref(m, 2).dtype == np.float16
    # feather: r = 0 is bin; all ones stays 255 under edge replication; all zeros stays 0
    assert np.array_equal(R.mask_feather_ref(m, 0), np.where(m >= 128, 255, 0))
    for r in R.RADII:
        assert (R.mask_feather_ref(np.full((2, 8, 8), 255, np.uint8), r) == 255).all() and (R.mask_feather_ref(np.zeros((2, 8, 8), np.uint8), r) == 0).all()
    # a half plane (columns 0 .. 3 on), r = 1, A = 9: column 3 sees 6 of 9 pixels on -> (6 * 255 + 4) / 9 = 170; columns 0 .. 2 see 9 -> 255; outside stays 0
    half = np.zeros((1, 6, 8), np.uint8)
    half[:, :, :4] = 255
    assert R.mask_feather_ref(half, 1)[0].tolist() == [[255, 255, 255, 170, 0, 0, 0, 0]] * 6
    # r = 3, A = 49: column c of the mask sees min(7, 4 + c... ) columns on: c = 0 -> columns -3 .. 3 (clamped: all on) = 7, c = 1 -> 6, c = 2 -> 5, c = 3 -> 4
    assert R.mask_feather_ref(half, 3)[0, 2].tolist() == [255, (6 * 7 * 255 + 24) // 49, (5 * 7 * 255 + 24) // 49, (4 * 7 * 255 + 24) // 49, 0, 0, 0, 0]
    # a single pixel keeps 255 / 9 rounded = 28 of itself at r = 1 and nothing outside itself
    one = np.zeros((1, 5, 5), np.uint8)
    one[0, 2, 2] = 255
    f1 = R.mask_feather_ref(one, 1)
    assert f1[0, 2, 2] == (255 + 4) // 9 == 28 and f1.sum() == 28
    # composite: the endpoints are exact for every pair, the midpoint rounds to nearest
    e, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    e, b = e[None, ..., None], b[None, ..., None]
    assert np.array_equal(R.image_composite_ref(e, b, np.full((1, 256, 256), 255, np.uint8)), e)
    assert np.array_equal(R.image_composite_ref(e, b, np.zeros((1, 256, 256), np.uint8)), b)
    mid = R.image_composite_ref(np.array([[[[200, 0, 255]]]], np.uint8), np.array([[[[100, 255, 255]]]], np.uint8), np.array([[[128]]], np.uint8))
    assert mid.tolist() == [[[[(128 * 200 + 127 * 100 + 127) // 255, (127 * 255 + 127) // 255, 255]]]] == [[[[150, 127, 255]]]]


# ---- refusals that need no model ----------------------------------------------------------------------------------------------------------------------------
def test_float_outputs_are_refused_with_a_mask_before_anything_runs():
    from instructany2pix_amd.batch import edit_batch
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    never = lambda *a, **kw: pytest.fail("a refusal came after the conditioner was asked")
    stub = SimpleNamespace(vae=object(), ip_adapter_xl=object(), piperf=None, model=None, any2pix_lm=None, conditioner=never, _conditions_for_batch=never)
    mask = np.full((16, 16), 255, np.uint8)
    for ot in ("np", "pt"):
        with pytest.raises(ValueError, match='output_type must be "pil" or "latent"'):
            InstructAny2PixPipeline.__call__(stub, "a", [], output_type=ot, edit_mask=mask)
        with pytest.raises(ValueError, match='output_type must be "pil" or "latent"'):
            edit_batch(stub, ["a", "b"], [[], []], output_type=ot, edit_masks=[None, mask])
    with pytest.raises(ValueError, match="edit_feather must be an integer radius"):
        InstructAny2PixPipeline.__call__(stub, "a", [], edit_mask=mask, edit_feather=65)
    with pytest.raises(ValueError, match="edit_feather must be an integer radius"):
        edit_batch(stub, ["a"], [[]], edit_masks=mask, edit_feather=-1)
    with pytest.raises(ValueError, match="`edit_masks` has 3 entries for 2 requests"):
        edit_batch(stub, ["a", "b"], [[], []], edit_masks=[mask, None, None])


# ---- launch lists -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def known_log(log, monkeypatch):
    """the recording stand-ins of test_joint_loops_cpu.py, plus one for the selection launch"""
    from instructany2pix_amd import batch

    def known_blend_v(x, known, level, mask, out, out2=None):
        assert level.dtype == torch.int32 and tuple(level.shape) == (x.shape[0],) and tuple(mask.shape) == (x.shape[0], 1, HW, HW)
        assert known.shape[1:] == x.shape and int(level.max()) < known.shape[0]
        log.append(("known", x.shape[0], level.tolist(), out2 is not None))
        return out
    monkeypatch.setattr(batch, "known_blend_v", known_blend_v)
    return log


def _denoise_pipe(log):
    from instructany2pix_amd.scheduler import DDIMScheduler
    unet = RecordingUNet(log, 6)
    ipa = SimpleNamespace(get_image_embeds=lambda clip_image_embeds=None, mode=None: _image_tokens(clip_image_embeds.shape[0]))
    return SimpleNamespace(ip_adapter_xl=ipa, pipe=SimpleNamespace(unet=unet, scheduler=DDIMScheduler(), vae_scale_factor=8))


def _edit_requests(masks):
    from instructany2pix_amd.batch import EditRequest
    return [EditRequest(base_latents=torch.zeros(1, 4, HW, HW), latent_la=torch.zeros(32), num_inference_steps=n, cfg=4.0, noise=torch.ones(1, 4, HW, HW).half(),
                        edit_mask=m, **_embeds()) for n, m in zip(STEPS, masks)]


def test_a_group_without_masks_records_exactly_the_unmasked_launch_list(known_log):
    from instructany2pix_amd.batch import RefineRequest, denoise_batch, refine_batch
    from instructany2pix_amd.scheduler import EulerDiscreteScheduler
    out, inv = denoise_batch(_denoise_pipe(known_log), _edit_requests([None] * 3), group=4)
    assert out.shape == inv.shape == (3, 4, HW, HW)
    assert known_log == [("unet", 3), ("update", 3)] * 6 + [("unet", 6), ("update", 3)] * 6          # test_joint_loops_cpu.py's list: no selection launch
    del known_log[:]
    piperf = SimpleNamespace(unet=RecordingUNet(known_log, 5), scheduler=EulerDiscreteScheduler(), vae_scale_factor=8, config=SimpleNamespace(requires_aesthetics_score=True))
    reqs = [RefineRequest(latents=torch.zeros(1, 4, HW, HW), strength=s, noise=torch.ones(1, 4, HW, HW).half(), **_embeds()) for s in (0.3, 0.5, 1.0)]
    assert refine_batch(piperf, reqs, group=4, num_inference_steps=8).shape == (3, 4, HW, HW)
    assert known_log == [("update", 3)] + [("update", 3), ("unet", 6), ("update", 3)] * 8            # no blend launch


def test_a_group_with_a_mask_adds_one_selection_per_sampling_step_and_one_blend_per_refiner_step(known_log):
    """steps 6 / 4 / 5, the middle request without a mask: the inversion's launches stay (its trajectory rides on out2), the sampling start and every sampling
    iteration are followed by ONE selection over all three rows at each request's own level, written to both halves"""
    from instructany2pix_amd.batch import RefineRequest, denoise_batch, refine_batch
    from instructany2pix_amd.scheduler import EulerDiscreteScheduler, known_levels
    m = torch.zeros(1, 1, HW, HW)
    m[..., : HW // 2] = 1
    out, inv = denoise_batch(_denoise_pipe(known_log), _edit_requests([m, None, m]), group=4)
    assert out.shape == inv.shape == (3, 4, HW, HW)
    lv = known_levels(STEPS)
    want = [("unet", 3), ("update", 3)] * 6 + [("known", 3, lv[0], False)]
    for i in range(6):
        want += [("unet", 6), ("update", 3), ("known", 3, lv[i + 1], True)]
    assert known_log == want and lv[-1] == [0, 0, 0]
    # two groups of a call: the one without a mask runs the unmasked list
    del known_log[:]
    denoise_batch(_denoise_pipe(known_log), _edit_requests([m, None, None]), group=1, shard=False)
    first = 2 * STEPS[0] + 1 + 3 * STEPS[0]         # the masked group of one: inversion, the start selection, sampling with a selection per iteration
    assert [e[0] for e in known_log[:first]].count("known") == STEPS[0] + 1
    assert known_log[first:] == [("unet", 1), ("update", 1)] * STEPS[1] + [("unet", 2), ("update", 1)] * STEPS[1] + [("unet", 1), ("update", 1)] * STEPS[2] + \
        [("unet", 2), ("update", 1)] * STEPS[2]
    del known_log[:]
    piperf = SimpleNamespace(unet=RecordingUNet(known_log, 5), scheduler=EulerDiscreteScheduler(), vae_scale_factor=8, config=SimpleNamespace(requires_aesthetics_score=True))
    reqs = [RefineRequest(latents=torch.zeros(1, 4, HW, HW), strength=s, noise=torch.ones(1, 4, HW, HW).half(), **_embeds(),
                          **(dict(known_latents=torch.zeros(1, 4, HW, HW), edit_mask=m) if k != 1 else {})) for k, s in enumerate((0.3, 0.5, 1.0))]
    assert refine_batch(piperf, reqs, group=4, num_inference_steps=8).shape == (3, 4, HW, HW)
    assert known_log == [("update", 3), ("blend", 3)] + [("update", 3), ("unet", 6), ("update", 3), ("blend", 3)] * 8
    with pytest.raises(ValueError, match="go together"):
        refine_batch(piperf, [RefineRequest(latents=torch.zeros(1, 4, HW, HW), strength=0.5, noise=torch.ones(1, 4, HW, HW).half(), edit_mask=m, **_embeds())],
                     num_inference_steps=8)


def test_refine_tables_carry_the_blend_to_the_next_sigma():
    from instructany2pix_amd.batch import refine_tables
    from instructany2pix_amd.scheduler import EulerDiscreteScheduler
    cfg = EulerDiscreteScheduler().config
    tb = refine_tables(cfg, (0.3, 0.5, 1.0), 8, 5.0)
    sch = EulerDiscreteScheduler.from_config(cfg)
    sch.set_timesteps(8)
    assert len(tb.blend) == 8 and all(len(row) == 3 for row in tb.blend)
    for r, n in enumerate(tb.steps):
        t_start = 8 - n
        assert tb.start_sigma[r] == float(sch.sigmas[t_start])
        for k in range(8):
            assert tb.blend[k][r] == ((1.0, float(sch.sigmas[t_start + k + 1])) if k < n else (1.0, 0.0))
        assert tb.blend[n - 1][r] == (1.0, 0.0)     # after a request's last step the noise level is 0: the known latents themselves
        for k in range(n - 1):                      # the blend's sigma is where the Euler step arrives: sigma + (sigma_next - sigma)
            assert tb.blend[k][r][1] == float(sch.sigmas[t_start + k + 1]) and abs(tb.coef[k][r][2] - (tb.blend[k][r][1] - float(sch.sigmas[t_start + k]))) < 1e-6
