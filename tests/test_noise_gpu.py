"""The three seeded-noise launches (include/ia2p.h, "Seeded noise": ia2p_randn_seeded, ia2p_posterior_sample_seeded, ia2p_polar_mix_v) on the MI355X against the
float64 restatement of tests/noise_ref.py, each within the bound that file counts from the operations; the invariances the rule promises, bit for bit; guard
regions on both sides of every output. Then the pipeline level (section 8): a request's image follows from the request and its seed alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref  # noqa: E402
import sampler_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                      # elements kept on either side of an output
SENTINEL = -77.0
SEEDS = (0, 1, 0x0123456789ABCDEF, 2 ** 63 - 1)
WORST = {}                      # launch -> worst observed error / bound (printed; docs/LOG.md §30 records it)


def _guarded(n, dtype, skew=0):
    """-> (whole buffer, the n-element output view starting `skew` elements past a 16-byte boundary, check()) -- torch allocations are 256-byte aligned and
    GUARD elements are a multiple of 16 bytes"""
    buf = torch.full((GUARD + skew + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + skew:GUARD + skew + n]

    def check():
        assert bool((buf[:GUARD + skew] == SENTINEL).all()) and bool((buf[GUARD + skew + n:] == SENTINEL).all()), "a guard element was written"
    return buf, view, check


def _randn(seeds, draws, per, first=0, dtype=torch.float32, skew=0):
    """the raw launch into a guarded buffer -> [B, per] on the host"""
    from instructany2pix_amd import _ffi
    B = len(seeds)
    _, view, check = _guarded(B * per, dtype, skew)
    st = _ffi.lib().ia2p_randn_seeded(_ffi.current_stream(), C.c_void_p(view.data_ptr()), int(dtype == torch.float16), B, per, first,
                                      (C.c_uint64 * B)(*seeds), (C.c_uint32 * B)(*draws))
    _ffi.check(st)
    torch.cuda.synchronize()
    check()
    return view.reshape(B, per).cpu()


_REF = {}


def _ref(seed, draw, n, first=0):
    """float64 reference of a stream's first elements, computed once per (seed, draw) and shared"""
    key = (seed, draw)
    need = first + n
    if key not in _REF or _REF[key][0].size < need:
        _REF[key] = noise_ref.normals(seed, draw, max(need, 4096))
    z, r = _REF[key]
    return z[first:first + n], r[first:first + n]


def _row_seeds(B):
    return [SEEDS[b % 4] + (b // 4) for b in range(B)], [(1, 0, 3, 5)[b % 4] for b in range(B)]


# ---- 1. fp32 output against the float64 restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 4, 1020])
@pytest.mark.parametrize("B", [1, 3, 8, 9])
def test_randn_seeded_fp32_within_the_op_count_bound(B, first):
    seeds, draws = _row_seeds(B)
    for per in (1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1025, 4 * 16 * 16):
        for skew in (0, 1, 3):                  # rows that start 0, 4 and 12 bytes past a 16-byte boundary
            got = _randn(seeds, draws, per, first, torch.float32, skew).double().numpy()
            for b in range(B):
                z, r = _ref(seeds[b], draws[b], per, first)
                err, bound = np.abs(got[b] - z), noise_ref.normal_bound(r)
                ok = err <= bound
                assert ok.all(), (B, per, first, skew, b, int(np.argmin(ok)), float(err.max()))
                WORST["randn"] = max(WORST.get("randn", 0.0), float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    print(f"randn_seeded fp32 B={B} first={first}: worst error / bound so far {WORST['randn']:.3f}")


# ---- 2. fp16 output = the fp32 output rounded ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,per,first", [(1, 1, 0), (3, 7, 4), (8, 257, 0), (9, 1025, 1020), (3, 4 * 16 * 16, 0), (1, 8, 4)])
def test_randn_seeded_fp16_is_the_fp32_output_cast(B, per, first):
    seeds, draws = _row_seeds(B)
    f32 = _randn(seeds, draws, per, first, torch.float32)
    for skew in (0, 2, 6, 1):                   # 0, 4, 12 and 2 bytes past a 16-byte boundary
        f16 = _randn(seeds, draws, per, first, torch.float16, skew)
        assert torch.equal(f16, f32.half()), (B, per, first, skew)


# ---- 3. invariance, bit for bit --------------------------------------------------------------------------------------------------------------------
def test_randn_seeded_invariances():
    seeds, draws = _row_seeds(8)
    per = 1025
    full = _randn(seeds, draws, per)
    for r in range(8):                          # a row alone is the row in the batch
        assert torch.equal(_randn([seeds[r]], [draws[r]], per)[0], full[r]), r
    for m, p in ((1, 9), (64, 257), (255, 5)):  # a sub-range is the same elements
        assert torch.equal(_randn(seeds[:3], draws[:3], p, first=4 * m), full[:3, 4 * m:4 * m + p]), (m, p)
    for dtype, skews in ((torch.float32, (1, 3)), (torch.float16, (1, 2, 6))):
        want = _randn(seeds, draws, per, dtype=dtype)
        for skew in skews:                      # aligned and misaligned rows agree
            assert torch.equal(_randn(seeds, draws, per, dtype=dtype, skew=skew), want), (dtype, skew)
    a, b = _randn([7], [2], 4096), _randn([7], [3], 4096)
    assert not torch.equal(a, b) and float((a == b).float().mean()) < 0.01          # the draw id matters
    # the domain tag: the words behind (seed, draw 0) are not the sampler's blocks at the steps 0 .. n for the same seed
    seed = SEEDS[2]
    wa, _ = noise_ref.words(seed, 0, 0, 64)
    mine = {float(np.float32(int(w) >> 8) * np.float32(2.0 ** -24)) for w in wa}
    theirs = {float(sampler_ref.uniform(seed, step)) for step in range(64)}
    assert not (mine & theirs)
    z0 = _randn([seed], [0], 4)[0]
    u = float(sampler_ref.uniform(seed, 0))
    u1 = (int(u * 2 ** 24) + 1) * 2.0 ** -24     # what element 0 would be had it been drawn from the sampler's block at step 0
    w1 = sampler_ref.philox4x32_10((0, 0, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[1]
    as_sampler = np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * (w1 >> 8) * 2.0 ** -24)
    assert abs(float(z0[0]) - as_sampler) > 1e-3


# ---- 4. moments on the device ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_randn_seeded_fp16_moments(seed):
    from instructany2pix_amd.noise import randn_seeded
    n = 1 << 20
    z = randn_seeded([seed] * 3, [0, 1, 3], (n,), torch.float16, DEV).double().cpu().numpy()
    caps = noise_ref.moment_caps(n)
    for row, draw in enumerate((0, 1, 3)):
        got = noise_ref.moments4(z[row])
        print(f"seed {seed:#x} draw {draw}: mean {got[0]:.2e} var-1 {got[1] - 1:.2e} skew {got[2]:.2e} kurt {got[3]:.2e} max {got[4]:.3f}")
        assert abs(got[0]) < caps[0] and abs(got[1] - 1) < caps[1] and abs(got[2]) < caps[2] and abs(got[3]) < caps[3] and got[4] <= caps[4], (seed, draw, got)


# ---- 5. the posterior sample -----------------------------------------------------------------------------------------------------------------------
def _posterior(mom, seeds, draw, sf):
    from instructany2pix_amd import _ffi
    B, C2, HW = mom.shape
    _, min_view, check_in = _guarded(mom.numel(), torch.float16)
    min_view.copy_(mom.reshape(-1))
    _, view, check = _guarded(B * (C2 // 2) * HW, torch.float16)
    _ffi.check(_ffi.lib().ia2p_posterior_sample_seeded(_ffi.current_stream(), C.c_void_p(min_view.data_ptr()), C.c_void_p(view.data_ptr()), B, C2 // 2, HW, sf,
                                                       (C.c_uint64 * B)(*seeds), (C.c_uint32 * B)(*[draw] * B)))
    torch.cuda.synchronize()
    check()
    check_in()
    return view.reshape(B, C2 // 2, HW).cpu()


@pytest.mark.parametrize("HW", [16, 35, 256])
@pytest.mark.parametrize("B", [1, 3])
def test_posterior_sample_seeded_within_the_op_count_bound(B, HW):
    Cc = 4
    g = torch.Generator().manual_seed(100 * B + HW)
    mom = torch.cat([torch.randn(B, Cc, HW, generator=g), torch.randn(B, Cc, HW, generator=g) * 3 - 2], dim=1)
    mom[:, Cc, 0], mom[:, Cc + 1, 1], mom[:, Cc + 2, HW - 1], mom[:, Cc + 3, 2] = -40.0, 25.0, -31.0, 21.0      # log-variances outside [-30, 20]
    mom = mom.half().to(DEV)
    seeds = [SEEDS[(b + 2) % 4] for b in range(B)]
    for sf in (0.13025, 0.18215):
        got = _posterior(mom, seeds, 0, sf)
        x64, bound = noise_ref.posterior(mom.cpu().numpy(), seeds, 0, sf)
        want = x64 * float(np.float32(sf))
        inside = np.abs(x64) < noise_ref.F16_MAX * (1 - 2.0 ** -10)          # an fp16 result that is certainly finite
        err = np.abs(got.double().numpy() - want)
        assert inside.mean() > 0.9 and (err[inside] <= bound[inside]).all(), (B, HW, sf, float((err[inside] / bound[inside]).max()))
        over = np.abs(x64) > noise_ref.F16_MAX * (1 + 2.0 ** -10)            # std = exp(10) at the clamp: the reference's fp16 cast overflows too
        assert (np.isinf(got.numpy()[over]) & (np.sign(got.numpy()[over]) == np.sign(x64[over]))).all()
        WORST["posterior"] = max(WORST.get("posterior", 0.0), float((err[inside] / bound[inside]).max()))
        # the clamps are taken: at logvar -40 the sample is its mean to fp16 rounding, at +25 its spread is exp(10), not exp(12.5)
        m64 = mom.cpu().double().numpy()
        assert np.allclose(x64[:, 0, 0], m64[:, 0, 0], atol=6 * np.exp(-15.0))
        for b in range(B):                      # a row's bits do not depend on B
            assert torch.equal(_posterior(mom[b:b + 1], seeds[b:b + 1], 0, sf)[0], got[b]), (b, sf)
    assert not torch.equal(_posterior(mom, seeds, 2, 0.13025), got)
    print(f"posterior_sample_seeded B={B} HW={HW}: worst error / bound so far {WORST['posterior']:.3f}")


# ---- 6. polar mixing -------------------------------------------------------------------------------------------------------------------------------
def _mix(x, y, alphas):
    from instructany2pix_amd import _ffi
    B, per = x.shape
    _, view, check = _guarded(B * per, torch.float16)
    _ffi.check(_ffi.lib().ia2p_polar_mix_v(_ffi.current_stream(), _ffi.ptr(x), _ffi.ptr(y), (C.c_float * B)(*alphas), C.c_void_p(view.data_ptr()), B, per))
    torch.cuda.synchronize()
    check()
    return view.reshape(B, per).cpu()


@pytest.mark.parametrize("per", [140, 256, 1024])
@pytest.mark.parametrize("B", [1, 3])
def test_polar_mix_v_within_the_op_count_bound(B, per):
    g = torch.Generator().manual_seed(7 * B + per)
    x, y = (torch.randn(B, per, generator=g) * 1.7).half().to(DEV), torch.randn(B, per, generator=g).half().to(DEV)
    for alpha in (0.0, 0.5, 0.7, 1.0):
        got = _mix(x, y, [alpha] * B)
        for b in range(B):
            want, bound = noise_ref.polar(x[b].cpu().numpy(), y[b].cpu().numpy(), alpha)
            err = np.abs(got[b].double().numpy() - want)
            assert (err <= bound).all(), (B, per, alpha, b, float((err / bound).max()))
            WORST["polar"] = max(WORST.get("polar", 0.0), float((err / bound).max()))
        if alpha == 1.0:                        # x rescaled by n0 / |x|: x itself within rounding
            assert torch.allclose(got.float(), x.cpu().float(), rtol=2.0 ** -10, atol=0)
    # a row's bits depend on neither B nor its place
    alphas = [0.7, 0.5, 0.25][:B]
    got = _mix(x, y, alphas)
    for b in range(B):
        assert torch.equal(_mix(x[b:b + 1].contiguous(), y[b:b + 1].contiguous(), alphas[b:b + 1])[0], got[b]), b
    if B == 3:
        perm = [2, 0, 1]
        moved = _mix(x[perm].contiguous(), y[perm].contiguous(), [alphas[i] for i in perm])
        for to, frm in enumerate(perm):
            assert torch.equal(moved[to], got[frm])
    print(f"polar_mix_v B={B} per={per}: worst error / bound so far {WORST['polar']:.3f}")


def test_polar_mix_v_more_rows_than_ride_by_value_whole_slices_and_zero_norm():
    g = torch.Generator().manual_seed(5)
    per = 4 * 64 * 64                           # two slices of 8192: two workgroups per row
    x, y = torch.randn(9, per, generator=g).half().to(DEV), torch.randn(9, per, generator=g).half().to(DEV)
    alphas = [0.1 * (b + 1) for b in range(9)]
    got = _mix(x, y, alphas)
    for b in (0, 7, 8):
        want, bound = noise_ref.polar(x[b].cpu().numpy(), y[b].cpu().numpy(), alphas[b])
        assert (np.abs(got[b].double().numpy() - want) <= bound).all(), b
        assert torch.equal(_mix(x[b:b + 1].contiguous(), y[b:b + 1].contiguous(), alphas[b:b + 1])[0], got[b]), b
    zero = _mix(torch.zeros(1, 64, dtype=torch.float16, device=DEV), torch.zeros(1, 64, dtype=torch.float16, device=DEV), [0.7])
    assert not torch.isfinite(zero.float()).any()          # |ll| = 0: the reference's 0 / 0, not an error
    from instructany2pix_amd.noise import polar_mix
    from instructany2pix_amd.pipeline import polar_intrtpolate
    ref = polar_intrtpolate(x[:1].cpu().float(), y[:1].cpu().float(), 0.7)
    assert torch.allclose(polar_mix(x[:1].reshape(1, 4, 64, 64), y[:1].reshape(1, 4, 64, 64), 0.7).cpu().float().reshape(1, -1), ref, rtol=2e-3, atol=1e-3)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_launch_nothing():
    from instructany2pix_amd import _ffi
    L, s = _ffi.lib(), _ffi.current_stream()
    out = torch.full((2, 64), 5.0, dtype=torch.float32, device=DEV)
    h = torch.full((2, 64), 5.0, dtype=torch.float16, device=DEV)
    mom = torch.zeros(2, 8, 8, dtype=torch.float16, device=DEV)
    seeds, draws, alphas = (C.c_uint64 * 2)(1, 2), (C.c_uint32 * 2)(0, 0), (C.c_float * 2)(0.5, 0.5)
    p = _ffi.ptr
    assert L.ia2p_randn_seeded(s, None, 0, 2, 64, 0, seeds, draws) == 1                       # IA2P_ERR_INVALID: a null pointer
    assert L.ia2p_randn_seeded(s, p(out), 0, 2, 64, 0, None, draws) == 1
    assert L.ia2p_randn_seeded(s, p(out), 0, 2, 64, 0, seeds, None) == 1
    assert L.ia2p_randn_seeded(s, p(out), 0, 0, 64, 0, seeds, draws) == 2                     # IA2P_ERR_SHAPE
    assert L.ia2p_randn_seeded(s, p(out), 0, 2, 0, 0, seeds, draws) == 2
    assert L.ia2p_randn_seeded(s, p(out), 0, 2, 64, 2, seeds, draws) == 2                     # first % 4 != 0
    assert L.ia2p_randn_seeded(s, p(out), 0, 2, 64, 2 ** 34 - 60, seeds, draws) == 2          # first + per > 2^34
    assert L.ia2p_randn_seeded(s, p(out), 0, 1, 2 ** 34 + 4, 0, seeds, draws) == 2
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_randn_seeded(s, p(out), 0, 2, 64, 2, seeds, draws))
    for i in range(2):
        a = [p(mom), p(h)]
        a[i] = None
        assert L.ia2p_posterior_sample_seeded(s, *a, 2, 4, 8, 1.0, seeds, draws) == 1
    assert L.ia2p_posterior_sample_seeded(s, p(mom), p(h), 2, 4, 8, 1.0, None, draws) == 1
    for B, Cc, HW in ((0, 4, 8), (2, 0, 8), (2, 4, 0)):
        assert L.ia2p_posterior_sample_seeded(s, p(mom), p(h), B, Cc, HW, 1.0, seeds, draws) == 2
    for i in range(4):
        a = [p(h), p(h), alphas, p(h)]
        a[i] = None
        assert L.ia2p_polar_mix_v(s, *a, 2, 64) == 1
    assert L.ia2p_polar_mix_v(s, p(h), p(h), alphas, p(h), 0, 64) == 2
    assert L.ia2p_polar_mix_v(s, p(h), p(h), alphas, p(h), 2, 0) == 2
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((h == 5.0).all())                                # no refused call launched anything
    assert L.ia2p_randn_seeded(s, p(out), 0, 2, 64, 2 ** 34 - 64, seeds, draws) == 0          # the last 64 elements of a stream are served
    torch.cuda.synchronize()
    want, _ = noise_ref.normals(1, 0, 64, first=2 ** 34 - 64)
    assert np.abs(out[0].double().cpu().numpy() - want).max() < 1e-5


# ---- 8. pipeline level: tiny configs, 16 x 16 latents, the conditioners supply no noise ------------------------------------------------------------
from test_edit_batch_gpu import Models, _cond, _traj  # noqa: E402

NOISES = ("polar_noise", "refiner_noise", "subject_noise")
KW = dict(num_inference_steps=3, cfg=4.0, refinement=0.1, subject_strength=0.1, group=4)          # 3 DDIM steps each way, 5 refiner steps, 5 steps per subject pass


@pytest.fixture(scope="module")
def models():
    return Models()


def _conds(models, first, n, n_subjects=2, keep=()):
    conds = {f"edit {first + i}": _cond(models, first + i, n_subjects=n_subjects) for i in range(n)}
    for c in conds.values():
        for k in NOISES:
            if k not in keep:
                del c[k]
    return conds


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.fixture(scope="module")
def served(models):
    """four seeded requests (two subjects each) through one `edit_batch`, latent hand-off: shared by the tests below and left unchanged"""
    conds = _conds(models, 200, 8)
    pipe = models.pipeline(conds, refiner_handoff="latent")
    insts, seeds = list(conds), [1000 + 17 * i for i in range(8)]
    torch.manual_seed(1)
    out = pipe.edit_batch(insts[:4], [[]] * 4, seeds=seeds[:4], **KW)
    assert all(msg == "SUCCESS!" for _, _, msg in out)
    return pipe, conds, insts, seeds, out


def test_edit_batch_seeds_fix_every_draw_whatever_the_global_generator_holds(models):
    """(a) the reference's hand-off through the tiny VAE, base images as PIL: every draw id is exercised (0 and 2 are the posterior samples)"""
    import PIL.Image
    conds = _conds(models, 300, 3, n_subjects=1)
    g = torch.Generator().manual_seed(9)
    for c in conds.values():
        del c["base_latents"]
        c["base_image"] = PIL.Image.fromarray(torch.randint(0, 256, (64, 64, 3), generator=g, dtype=torch.uint8).numpy())
        c["subject_data"] = [(torch.nn.functional.interpolate(mk[None, None], size=(64, 64))[0, 0], e) for mk, e in c["subject_data"]]
    pipe = models.pipeline(conds, vae=models.vae)
    assert pipe.refiner_handoff == "image"
    insts = list(conds)
    torch.manual_seed(11)
    a = pipe.edit_batch(insts, [[]] * 3, seeds=[5, 6, 7], debug=True, **KW)
    torch.manual_seed(12)
    b = pipe.edit_batch(insts, [[]] * 3, seeds=[5, 6, 7], **KW)
    for x, y in zip(a, b):
        assert _same(x, y) and not torch.equal(x[0], x[1])
    assert [x[2]["seed"] for x in a] == [5, 6, 7] and b[0][2] == "SUCCESS!"
    one = pipe.edit_batch(insts, [[]] * 3, seeds=5, **KW)                    # one int: seed + i
    assert all(_same(x, y) for x, y in zip(a, one))
    torch.manual_seed(11)
    free = pipe.edit_batch(insts, [[]] * 3, **KW)                            # unseeded: the global generator, as ever
    torch.manual_seed(12)
    free2 = pipe.edit_batch(insts, [[]] * 3, **KW)
    assert not torch.equal(free[0][0], free2[0][0]) and not torch.equal(free[0][0], a[0][0])
    with pytest.raises(ValueError):
        pipe.edit_batch(insts, [[]] * 3, seeds=[5, 6], **KW)


def test_a_request_keeps_its_bits_next_to_other_requests_and_at_another_place(served):
    """(b) request 0 with its seed: in a group of 4 next to requests 1..3, and at place 2 next to requests 4..6 with other seeds"""
    pipe, conds, insts, seeds, out = served
    order = [4, 5, 0, 6]
    torch.manual_seed(2)
    moved = pipe.edit_batch([insts[i] for i in order], [[]] * 4, seeds=[seeds[i] for i in order], **KW)
    assert _same(moved[2], out[0])
    assert not torch.equal(moved[0][1], out[1][1])


def test_call_with_the_seed_serves_the_same_request_from_the_same_noise(served, monkeypatch):
    """(c) `__call__(seed=s)` against the request's `edit_batch` row: the batch-against-serial bar of tests/test_edit_batch_gpu.py; its three kinds of
    noise are `randn_seeded` at the table's draw ids"""
    from instructany2pix_amd import noise
    pipe, conds, insts, seeds, out = served
    drawn, real = [], noise.randn_seeded

    def spy(s, d, shape, *a, **kw):
        t = real(s, d, shape, *a, **kw)
        drawn.append((list(s), d, t.clone()))
        return t
    monkeypatch.setattr(noise, "randn_seeded", spy)
    kw = {k: v for k, v in KW.items() if k != "group"}
    torch.manual_seed(3)
    nr, oo, msg = pipe(insts[1], [], seed=seeds[1], debug=True, **kw)
    monkeypatch.undo()
    pipe.ip_adapter_xl.set_scale(1.0)                # the serial inpaint `generate` leaves 0.8 on the shared processors
    assert msg["seed"] == seeds[1]
    for what, got, want in (("non_refined", nr, out[1][0]), ("oo", oo, out[1][1])):
        rel, cos = _traj(got, want)
        print(f"__call__(seed) vs edit_batch row, {what}: rel-L2 {rel:.3e} cos {cos:.6f}")
        assert rel < 3e-2 and cos > 0.999, (what, rel, cos)
    assert [(s, d) for s, d, _ in drawn] == [([seeds[1]], noise.DRAW_POLAR), ([seeds[1]], noise.DRAW_REFINER), ([seeds[1]], noise.DRAW_INPAINT),
                                             ([seeds[1]], noise.DRAW_INPAINT + 1)]
    for s, d, t in drawn:
        assert t.shape == (1, 4, 16, 16) and torch.equal(t, noise.randn_seeded(s, d, (4, 16, 16), torch.float16, DEV))
        z, _ = noise_ref.normals(s[0], d, 4 * 16 * 16)
        assert np.abs(t.double().cpu().numpy().ravel() - z).max() < 2.0 ** -9 + 2.0 ** -18      # (fp16 of a value below 8: half an ulp is 2^-9 at most)


def test_a_supplied_polar_noise_wins_over_the_seed(models):
    """(d)"""
    conds = _conds(models, 400, 2, n_subjects=0, keep=("polar_noise",))
    pipe = models.pipeline(conds, refiner_handoff="latent")
    kw = dict(KW, refinement=0.0, subject_strength=0.0)
    a = pipe.edit_batch(list(conds), [[]] * 2, seeds=[1, 2], **kw)
    b = pipe.edit_batch(list(conds), [[]] * 2, seeds=[101, 102], **kw)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b))
    for c in conds.values():
        del c["polar_noise"]
    c = pipe.edit_batch(list(conds), [[]] * 2, seeds=[1, 2], **kw)
    assert not torch.equal(c[0][0], a[0][0])


def test_seeded_and_unseeded_requests_share_a_group(served):
    """(e) the seeded rows keep their bits; the others follow the global generator"""
    pipe, conds, insts, seeds, out = served
    mixed = [seeds[0], None, seeds[2], None]
    torch.manual_seed(4)
    a = pipe.edit_batch(insts[:4], [[]] * 4, seeds=mixed, **KW)
    torch.manual_seed(5)
    b = pipe.edit_batch(insts[:4], [[]] * 4, seeds=mixed, debug=True, **KW)
    for i in (0, 2):
        assert _same(a[i], out[i]) and _same(b[i], out[i]), i
    for i in (1, 3):
        assert not torch.equal(a[i][0], b[i][0]) and not torch.equal(a[i][0], out[i][0]), i
    assert b[0][2]["seed"] == seeds[0] and "seed" not in b[1][2]


def test_seeded_denoise_keeps_the_latents_on_the_device(served, monkeypatch):
    """(f) what is handed to sampling lives on the device, and `polar_intrtpolate` is never called"""
    from instructany2pix_amd import pipeline as P
    from instructany2pix_amd.batch import EditRequest
    pipe, conds, insts, seeds, _ = served
    c = conds[insts[0]]

    def forbidden(*a, **kw):
        raise RuntimeError("polar_intrtpolate was called")
    monkeypatch.setattr(P, "polar_intrtpolate", forbidden)
    seen, real = [], pipe.ip_adapter_xl.generate

    def generate(*a, **kw):
        seen.append(kw["latents"])
        return real(*a, **kw)
    monkeypatch.setattr(pipe.ip_adapter_xl, "generate", generate)
    emb = {k: c[k] for k in ("prompt_embeds", "pooled_prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds")}
    la = torch.randn(64, generator=torch.Generator().manual_seed(1))
    images, inv = pipe.denoise(c["base_latents"], la, num_inference_steps=3, cfg=4.0, seed=77, **emb)
    assert len(seen) == 1 and seen[0].is_cuda and seen[0].dtype == torch.float16 and images.shape == (1, 4, 16, 16) and torch.isfinite(images.float()).all()
    again, _ = pipe.denoise(c["base_latents"], la, num_inference_steps=3, cfg=4.0, seed=77, **emb)
    other, _ = pipe.denoise(c["base_latents"], la, num_inference_steps=3, cfg=4.0, seed=78, **emb)
    assert torch.equal(again, images) and not torch.equal(other, images)
    with pytest.raises(RuntimeError, match="polar_intrtpolate was called"):      # the unseeded call still mixes on the host
        pipe.denoise(c["base_latents"], la, num_inference_steps=3, cfg=4.0, **emb)
    reqs = [EditRequest(base_latents=c["base_latents"], latent_la=la, num_inference_steps=3, cfg=4.0, seed=77 + i, **emb) for i in range(2)]
    out, _ = pipe.denoise_batch(reqs, group=2)                                    # the batched hot segment likewise
    assert out.shape == (2, 4, 16, 16) and not torch.equal(out[0], out[1])
    with pytest.raises(RuntimeError, match="polar_intrtpolate was called"):
        pipe.denoise_batch([EditRequest(base_latents=c["base_latents"], latent_la=la, num_inference_steps=3, cfg=4.0, **emb)], group=2)


def test_two_seeds_give_two_images(served):
    """(g)"""
    pipe, conds, insts, seeds, out = served
    other = pipe.edit_batch(insts[:4], [[]] * 4, seeds=[s + 1 for s in seeds[:4]], **KW)
    for i in range(4):
        assert not torch.equal(other[i][0], out[i][0]) and not torch.equal(other[i][1], out[i][1]), i
