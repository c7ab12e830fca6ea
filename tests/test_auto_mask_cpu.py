"""Automatic edit masks without a GPU: the fp64 reference against hand cases, the mutants it has to separate, the error bound against the kernels' own
evaluation order replayed in float32, and the host logic -- knobs, noise level, draw ids, draw order, refusals before anything runs."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import auto_mask_ref as R                                  # noqa: E402


# ---- hand cases -----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_two_by_three_grid_by_hand():
    # n = 1, C = 2: map = (|t0 - s0| + |t1 - s1|) / 2
    tgt = np.array([[[[[1.0, 0.0, -2.0], [0.5, 0.0, 4.0]], [[1.0, 0.0, 2.0], [0.5, 1.0, 0.0]]]]])      # [1, 1, 2, 2, 3]
    src = np.array([[[[[0.0, 0.0, 2.0], [0.5, 0.0, 0.0]], [[-1.0, 0.0, 2.0], [0.0, 0.0, 0.0]]]]])
    cmap, stats, m, mask = R.auto_mask_ref(tgt, src, ratio=2.0, dilate=0)
    assert cmap.tolist() == [[[1.5, 0.0, 2.0], [0.25, 0.5, 2.0]]]
    assert stats.tolist() == [[6.25 / 6, 6.25 / 6]]                                  # ratio 2: tau = mean
    assert m.tolist() == [[[True, False, True], [False, False, True]]] and mask.dtype == np.float16 and mask.shape == (1, 1, 2, 3)
    assert mask[0, 0].tolist() == [[1, 0, 1], [0, 0, 1]]                             # d = 0: the identity
    assert R.auto_mask_ref(tgt, src, 2.0, 1)[3].all()                                # d = 1 on 2 x 3: every cell has an on neighbour
    assert R.auto_mask_ref(tgt, src, 3.0, 0)[2].tolist() == [[[False, False, True], [False, False, True]]]      # tau = 1.5625


def test_ties_at_tau_give_zero_and_equal_predictions_an_empty_mask():
    tgt, src = R.tie_case(2, 4, 8, 8)
    cmap, stats, m, mask = R.auto_mask_ref(tgt, src, 3.0, 0)
    assert stats.tolist() == [[0.5, 0.75]] and (cmap == 0.75).sum() == 24            # 24 cells sit exactly on tau
    assert not m[cmap == 0.75].any() and m[cmap == 1.5].all() and m.sum() == 8       # strict: the ties are off
    same = np.ones((2, 3, 4, 5, 7), np.float16)
    cmap, stats, m, mask = R.auto_mask_ref(same, same, 3.0, 2)
    assert not cmap.any() and not stats.any() and not mask.any() and np.isfinite(stats).all()      # mean = 0: 0 > 0 is false everywhere


def test_dilation_at_corners_and_across_a_row_end():
    m = np.zeros((1, 4, 5), bool)
    m[0, 0, 0] = True                                                                # a corner
    assert R.dilate_ref(m, 1)[0].astype(int).tolist() == [[1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    m = np.zeros((1, 4, 5), bool)
    m[0, 1, 4] = True                                                                # a row end: cell (2, 0) follows it in memory and stays 0
    assert R.dilate_ref(m, 1)[0].astype(int).tolist() == [[0, 0, 0, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 0, 0]]
    assert R.dilate_ref(m, 0)[0].sum() == 1 and R.dilate_ref(m, 4)[0].all()
    two = np.zeros((2, 3, 3), bool)
    two[:, 1, 1] = True
    out = R.dilate_ref(two, [0, 1])                                                  # one d per request
    assert out[0].sum() == 1 and out[1].all()
    assert not R.dilate_ref(np.zeros((1, 3, 3), bool), 2).any()                      # outside cells count 0: nothing grows out of an empty grid


# ---- mutants: each wrong rule must differ from the reference on the shared cases ----------------------------------------------------------------------------
def _wrap_dilate(m, d):
    B, h, w = m.shape
    flat = m.reshape(B, -1)
    out = np.zeros_like(flat)
    y, p = np.divmod(np.arange(h * w), w)[0], np.arange(h * w)
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            q = p + dy * w + dx                                # flat offset: a row end runs into the next row
            ok = (y + dy >= 0) & (y + dy < h) & (q >= 0) & (q < h * w)
            out[:, ok] |= flat[:, q[ok]]
    return out.reshape(B, h, w)


def _ones_outside_dilate(m, d):
    B, h, w = m.shape
    pad = np.ones((B, h + 2 * d, w + 2 * d), bool)
    pad[:, d:d + h, d:d + w] = m
    out = np.zeros_like(m)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            out |= pad[:, dy:dy + h, dx:dx + w]
    return out


def _mutant(name, tgt, src, ratio, d):
    t, s = tgt.astype(np.float64), src.astype(np.float64)
    nC = t.shape[1] * t.shape[2]
    cmap = R.contrast_map_ref(t, s)
    if name == "abs of each":
        cmap = np.abs(np.abs(t) - np.abs(s)).sum(axis=(1, 2)) / nC
    if name == "abs after the sum":
        cmap = np.abs((t - s).sum(axis=(1, 2))) / nC
    B = cmap.shape[0]
    mean = cmap.reshape(B, -1).mean(axis=1)
    if name == "batch mean":
        mean = np.full(B, cmap.mean())
    tau = (1.0 if name == "0.5 forgotten" else 0.5) * ratio * mean
    m = cmap >= tau[:, None, None] if name == ">=" else cmap > tau[:, None, None]
    if name == "wrap":
        return _wrap_dilate(m, d)
    if name == "outside is 1":
        return _ones_outside_dilate(m, d)
    return R.dilate_ref(m, d)


MUTANTS = ("abs of each", "abs after the sum", "batch mean", ">=", "0.5 forgotten", "wrap", "outside is 1")


def _shared_cases():
    cases = [R.real_case(*shape, seed=40 + i) + (3.0, 1) for i, shape in enumerate(R.REAL_CASES[:6])]
    cases.append(R.tie_case(2, 4, 8, 8) + (3.0, 0))
    t, s = R.real_case(2, 4, 4, 16, 16, seed=77)
    t[1], s[1] = t[1] * 0.25, s[1] * 0.25                      # two requests of different contrast: a batch mean is not theirs
    cases.append((t, s, 3.0, 1))
    return cases


def test_the_unmutated_rule_passes_through_the_mutant_harness():
    for t, s, ratio, d in _shared_cases():
        assert np.array_equal(_mutant("none", t, s, ratio, d), R.auto_mask_ref(t, s, ratio, d)[3][:, 0] != 0)


@pytest.mark.parametrize("name", MUTANTS)
def test_the_reference_separates_every_mutant(name):
    differs = [not np.array_equal(_mutant(name, t, s, ratio, d), R.auto_mask_ref(t, s, ratio, d)[3][:, 0] != 0) for t, s, ratio, d in _shared_cases()]
    assert any(differs), name


# ---- the bound, against the kernels' own order in float32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,shape", list(enumerate(R.REAL_CASES)))
def test_the_bound_covers_the_kernel_order_in_float32(i, shape):
    B, n, C, h, w = shape
    tgt, src = R.real_case(*shape, seed=100 + i)
    cmap, stats, m, _ = R.auto_mask_ref(tgt, src, 3.0, 0)
    got_map, got_stats = R.kernel_order_fp32(tgt, src, 3.0)
    bm, bmean, btau = R.bounds(cmap, stats, n * C)
    assert (np.abs(got_map - cmap) <= bm).all()
    assert (np.abs(got_stats[:, 0] - stats[:, 0]) <= bmean).all() and (np.abs(got_stats[:, 1] - stats[:, 1]) <= btau).all()
    sure = R.certain(cmap, stats, n * C)
    assert ((~sure).reshape(B, -1).sum(axis=1) <= R.max_uncertain(h * w)).all()
    got_m = got_map > got_stats[:, 1][:, None, None]
    assert np.array_equal(got_m[sure], m[sure])
    if h * w >= 63:
        on = m.reshape(B, -1).mean(axis=1)
        assert (on > 0.15).all() and (on < 0.55).all(), on          # amp uniform in [0, 4], tau = 1.5 mean: about the quarter of the cells with amp > 3


@pytest.mark.parametrize("shape", R.LATTICE_CASES)
def test_lattice_cases_are_exact_in_float32(shape):
    tgt, src = R.lattice_case(*shape, seed=7)
    cmap, stats, _, _ = R.auto_mask_ref(tgt, src, 3.0, 0)
    got_map, got_stats = R.kernel_order_fp32(tgt, src, 3.0)
    assert np.array_equal(got_map.astype(np.float64), cmap) and np.array_equal(got_stats.astype(np.float64), stats)


# ---- host logic ---------------------------------------------------------------------------------------------------------------------------------------------
def test_auto_mask_validates_itself():
    from instructany2pix_amd.auto_mask import AutoMask, resolve_auto_mask
    d = AutoMask()
    assert (d.num_maps, d.strength, d.ratio, d.dilate, d.noise, d.max_rows) == (8, 0.5, 3.0, 1, None, None)
    assert resolve_auto_mask(None) is None and resolve_auto_mask(False) is None and resolve_auto_mask(True) == d
    assert resolve_auto_mask(dict(num_maps=2, dilate=0)) == AutoMask(num_maps=2, dilate=0) and resolve_auto_mask(d) is d
    for kw, words in ((dict(num_maps=0), "num_maps=0 must be an integer in 1 .. 64"), (dict(num_maps=2.0), "num_maps=2.0"), (dict(num_maps=65), "num_maps=65"),
                      (dict(strength=1.5), "strength should in \\[0.0, 1.0\\] but is 1.5"), (dict(strength=float("nan")), "strength should in"),
                      (dict(ratio=0.0), "ratio=0.0 must be finite and positive"), (dict(ratio=float("inf")), "ratio=inf"), (dict(ratio=-1), "ratio=-1"),
                      (dict(dilate=-1), "dilate=-1 must be an integer in 0 .. 16"), (dict(dilate=17), "dilate=17"), (dict(dilate=True), "dilate=True"),
                      (dict(max_rows=0), "max_rows=0 must be None or an integer in 1 .. 16"), (dict(max_rows=17), "max_rows=17"),
                      (dict(noise=torch.zeros(3, 4, 8, 8)), "noise must be a tensor \\[num_maps = 8, C, h, w\\]")):
        with pytest.raises(ValueError, match="auto_mask: .*" + words):
            AutoMask(**kw)
        with pytest.raises(ValueError, match=words + ".* \\(request 2\\)"):          # several requests share a call: the message names the request
            resolve_auto_mask(kw, " (request 2)")
    with pytest.raises(ValueError, match="unknown keys \\['maps'\\] \\(request 0\\)"):
        resolve_auto_mask(dict(maps=3), " (request 0)")
    with pytest.raises(ValueError, match="must be None, True, a dict"):
        resolve_auto_mask(3)


@pytest.mark.parametrize("N,s", [(25, 0.5), (4, 0.5), (3, 1.0), (5, 0.2)])
def test_the_noise_level_is_the_first_kept_timestep(N, s):
    from instructany2pix_amd.auto_mask import auto_mask_timestep
    from instructany2pix_amd.scheduler import DDIMScheduler, kept_steps
    sch = DDIMScheduler()
    sch.set_timesteps(N)
    t_start, kept = kept_steps(N, s)
    assert kept >= 1 and auto_mask_timestep(sch.config, N, s) == int(sch.timesteps[t_start])
    by_hand = {(25, 0.5): 13, (4, 0.5): 2, (3, 1.0): 0, (5, 0.2): 4}[(N, s)]        # N - int(N s)
    assert t_start == by_hand and int(sch.timesteps[by_hand]) == (N - 1 - by_hand) * (1000 // N) + 1


def test_a_strength_that_keeps_no_step_is_refused_in_the_schedulers_words():
    from instructany2pix_amd.auto_mask import auto_mask_timestep
    from instructany2pix_amd.scheduler import DDIMScheduler
    cfg = DDIMScheduler().config
    with pytest.raises(ValueError, match="After adjusting the num_inference_steps by strength parameter: 0.1, the number of pipeline steps is 0 which is < 1.* \\(request 1\\)"):
        auto_mask_timestep(cfg, 4, 0.1, " (request 1)")
    with pytest.raises(ValueError, match="`num_inference_steps` has to be a positive integer but is 0"):
        auto_mask_timestep(cfg, 0, 0.5)


def test_the_draw_id_collides_with_no_other_draw():
    from instructany2pix_amd import noise
    assert noise.DRAW_AUTO_MASK == 1 << 16
    others = {noise.DRAW_BASE_POSTERIOR, noise.DRAW_POLAR, noise.DRAW_HANDOFF_POSTERIOR, noise.DRAW_REFINER}
    assert others == {0, 1, 2, 3} and noise.DRAW_AUTO_MASK not in others
    ids = {noise.inpaint_draw(k) for k in range(65532)}
    assert len(ids) == 65532 and noise.DRAW_AUTO_MASK not in ids and max(ids) == noise.DRAW_AUTO_MASK - 1
    assert noise.check_draw(noise.DRAW_AUTO_MASK) == 65536
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ia2p.h")).read()
    assert "65536 = 1 << 16 the n noises of an" in hdr                                # the draw-id table of the header


def test_unseeded_draws_come_in_request_order_and_seeded_or_supplied_ones_draw_nothing():
    from instructany2pix_amd.auto_mask import AutoMask, estimate_noises
    lat = [torch.zeros(1, 4, 8, 8)] * 4
    given = torch.ones(3, 4, 8, 8).half()
    knobs = [AutoMask(num_maps=2), None, AutoMask(num_maps=3, noise=given), AutoMask(num_maps=1)]
    torch.manual_seed(11)
    got = estimate_noises(knobs, lat, [None, None, None, None])
    after = torch.randn(1)
    torch.manual_seed(11)
    first, last = torch.randn(2, 4, 8, 8, dtype=torch.float16), torch.randn(1, 4, 8, 8, dtype=torch.float16)      # request 0, then request 3: nothing in between
    assert torch.equal(got[0], first) and got[1] is None and got[2] is given and torch.equal(got[3], last) and torch.equal(after, torch.randn(1))
    torch.manual_seed(11)
    state = torch.get_rng_state()
    got = estimate_noises(knobs, lat, [5, None, 6, 7])                               # seeded: made on the device later, nothing drawn here
    assert got[0] is None and got[2] is given and got[3] is None and torch.equal(torch.get_rng_state(), state)
    assert estimate_noises([None] * 4, lat, [None] * 4) == [None] * 4 and torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="noise is \\(3, 4, 8, 8\\), expected \\(3, 4, 16, 16\\) \\(request 0\\)"):
        estimate_noises([knobs[2]], [torch.zeros(1, 4, 16, 16)], [None])


def test_the_polar_draw_follows_the_estimate_draw_in_denoise_batch(monkeypatch):
    """`denoise_batch`: the estimates' host draws (request order) come before the first polar-mixing draw"""
    from instructany2pix_amd import auto_mask as A
    from instructany2pix_amd import batch
    order = []
    z = lambda: torch.zeros(1, 4, 8, 8)
    reqs = [batch.EditRequest(z(), torch.zeros(8), z(), z(), z(), z(), num_inference_steps=4, cfg=4.0, auto_mask=a) for a in (True, None, dict(num_maps=2))]

    def estimate_group(pipeline, rs, knobs, noises, max_rows):
        order.append(("estimate", [k.num_maps for k in knobs], [tuple(n.shape) for n in noises], max_rows))
        return [A.AutoMaskEstimate(torch.ones(1, 1, 8, 8).half(), torch.zeros(1, 8, 8), torch.zeros(2), 0) for _ in rs]

    def host_noises(given, shapes, seeds, generator=None):
        order.append(("polar", len(given)))
        return [torch.zeros(tuple(s)).half() for s in shapes]

    def run_groups(requests, like, unet, group, shard, run_group, n_out=1):
        order.append(("groups", [r.auto_mask for r in requests], [None if r.edit_mask is None else tuple(r.edit_mask.shape) for r in requests]))
        return None, None
    monkeypatch.setattr(A, "estimate_group", estimate_group)
    monkeypatch.setattr(batch._noise, "host_noises", host_noises)
    monkeypatch.setattr(batch, "_run_groups", run_groups)
    monkeypatch.setattr(batch, "_denoise_group", lambda *a, **k: None)
    cfg = SimpleNamespace(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading",
                          set_alpha_to_one=False, prediction_type="epsilon", clip_sample=False)
    unet = SimpleNamespace(device="cpu")
    pipe = SimpleNamespace(ip_adapter_xl=object(), pipe=SimpleNamespace(unet=unet, scheduler=SimpleNamespace(config=cfg), vae_scale_factor=8))
    batch.denoise_batch(pipe, reqs, group=4)
    assert order[0] == ("estimate", [8, 2], [(8, 4, 8, 8), (2, 4, 8, 8)], 8)         # requests 0 and 2 as one group, 2 x group rows per evaluation
    assert order[1] == ("polar", 3)
    assert order[2] == ("groups", [None, None, None], [(1, 1, 8, 8), None, (1, 1, 8, 8)])      # the estimates went in as edit masks; request 1 as it was
    assert reqs[0].auto_mask is True and reqs[0].edit_mask is None                   # the caller's requests are not written to


def test_refusals_come_before_the_conditioner_is_asked():
    from instructany2pix_amd.batch import edit_batch
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    never = lambda *a, **kw: pytest.fail("a refusal came after the conditioner was asked")
    stub = SimpleNamespace(vae=object(), ip_adapter_xl=object(), piperf=None, model=None, any2pix_lm=None, conditioner=never, _conditions_for_batch=never)
    for ot in ("np", "pt"):
        with pytest.raises(ValueError, match='output_type must be "pil" or "latent"'):
            InstructAny2PixPipeline.__call__(stub, "a", [], output_type=ot, auto_mask=True)
        with pytest.raises(ValueError, match='output_type must be "pil" or "latent"'):
            edit_batch(stub, ["a", "b"], [[], []], output_type=ot, auto_masks=[None, True])
    with pytest.raises(ValueError, match="edit_feather must be an integer radius"):
        InstructAny2PixPipeline.__call__(stub, "a", [], auto_mask=True, edit_feather=65)
    with pytest.raises(ValueError, match="dilate=40"):
        InstructAny2PixPipeline.__call__(stub, "a", [], auto_mask=dict(dilate=40))
    with pytest.raises(ValueError, match="the number of pipeline steps is 0"):
        InstructAny2PixPipeline.__call__(stub, "a", [], num_inference_steps=4, auto_mask=dict(strength=0.1))
    with pytest.raises(ValueError, match="ratio=0 must be finite and positive \\(request 1\\)"):
        edit_batch(stub, ["a", "b"], [[], []], auto_masks=[None, dict(ratio=0)])
    with pytest.raises(ValueError, match="the number of pipeline steps is 0.* \\(request 0\\)"):
        edit_batch(stub, ["a", "b"], [[], []], num_inference_steps=[3, 25], refinement=0.0, auto_masks=dict(strength=0.2))
    with pytest.raises(ValueError, match="`auto_masks` has 3 entries for 2 requests"):
        edit_batch(stub, ["a", "b"], [[], []], auto_masks=[True, None, None])
    with pytest.raises(TypeError):
        InstructAny2PixPipeline.__call__(stub, "a", [], 0.7, [0.0, 0.4, 1.0], 20.0, 0.5, False, 25, False, False, "default", 0.0, 10, 1.0, "latent", None, None, 8, True)      # keyword only
