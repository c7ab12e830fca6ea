"""What tests/test_unet_ops_gpu.py rests on, checked without a GPU: the references of tests/unet_ops_ref.py against independent torch code in fp64 (a wrong reference
cannot bless a wrong kernel); the conditions under which "exact" is true, for every case the GPU file uses (the case lists are the reference module's); the cap on the
one modelled term (the native exponential: below a tenth of every SiLU bound); MUTANTS -- reference outputs perturbed the way a subtly wrong kernel would perturb them,
each of which the very comparison the GPU tests call (`accept`) must reject; and the host-side refusals of the entry points the GPU file goes through."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ops_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _close(a, b, tol=1e-12):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _tight(bound, ref, slack):
    """a bound is an fp16 rounding and a few fp32 roundings of the operands' magnitude (slack, relative to 1 + |ref|): not a tolerance"""
    ref = R.f64(ref)
    assert bool((R.f64(bound) <= 2 * R.half_ulp16(ref.abs()) + slack * (1 + ref.abs())).all()), float((R.f64(bound) - 2 * R.half_ulp16(ref.abs())).max())


def _rejected(tag, mutant, ref, bound=None):
    """the mutant differs from the reference and `accept` refuses it"""
    assert R.accept(tag + " (the reference itself)", ref if bound is not None else ref.clone(), ref, bound) <= 1.0
    with pytest.raises(AssertionError, match="worst at"):
        R.accept(tag, mutant, ref, bound)


ALL_GEMM = [R.gemm_case(*s) for s in R.GEMM_SHAPES] + [R.gemm_case(*s[:3]) for s in R.SPLITK_SHAPES]


# ---- the references against torch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL_GEMM, ids=lambda c: f"{c['M']}x{c['N']}x{c['K']}")
def test_gemm_reference_is_linear_with_two_roundings(c):
    acc, h, h16, s, out = R.gemm_parts(c)
    assert torch.equal(h, F.linear(R.f64(c["A"]), R.f64(c["W"]), R.f64(c["bias"])))
    want = (F.linear(c["A"].double(), c["W"].double(), c["bias"].double()).half().double() + c["res"].double()).half()
    assert torch.equal(out, want.double()) and torch.equal(R.gemm_ref(c)[0], out)
    assert torch.equal(R.gemm_ref(c, "none")[0], F.linear(c["A"].double(), c["W"].double()).half().double())
    # both kinds of output occur at both rounding points, and one rounding of the whole sum is another result
    assert bool((h != h16).any()) and bool((h == h16).any()) and bool((s != out).any()) and bool((s == out).any())
    assert float((R.round16(h + R.f64(c["res"])) != out).double().mean()) > 0.01
    # every column its own bias, every row its own residual level
    assert len(set(c["bias"].tolist())) == c["N"]
    lev = c["res"].double().mean(1)
    assert bool((lev[1:] - lev[:-1]).abs().min() > 0.25)


@pytest.mark.parametrize("shape", R.GEGLU_SHAPES)
def test_geglu_reference_is_value_times_gelu_of_the_gate(shape):
    c = R.geglu_case(*shape)
    ref, bound = R.geglu_ref(c)
    h = F.linear(c["A"].double(), c["W"].double(), c["bias"].double())
    assert torch.equal(h, R.round16(h)), "value and gate sums must be fp16 values"
    v, g = h.chunk(2, dim=-1)
    _close(ref, v * F.gelu(g))
    assert float(g.min()) <= -9 and float(g.max()) >= 9, "the gates must span [-9, 9]"
    inside = (g.abs() < 7.9)
    assert bool((bound[inside] <= 3.1e-5 * (v * g).abs()[inside] + 1.01 * R.half_ulp16(ref.abs() + 1e-3)[inside] + 1e-9).all())      # the table's 3e-5 and the store: not a tolerance
    # the table as gemm.hip builds it, interpolated in fp64, stays within the analytic part of the bound
    i, gc = R.lut_cell(g)
    x0 = (i - 256) / 32
    lut = R.phi(x0) + (gc * 32 + 256 - i) * (R.phi(x0 + 1 / 32) - R.phi(x0))
    assert R.accept("interpolated table", v * g * lut, ref, bound) <= 1.0


@pytest.mark.parametrize("shape", R.CONV_SHAPES)
def test_conv_reference_is_conv2d(shape):
    B, H, W, Cin, Co, stride, up = shape
    c = R.conv_case(*shape)
    xn = c["x"].double().permute(0, 3, 1, 2)
    if up:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    h = F.conv2d(xn, c["w"].double(), c["bias"].double(), stride=stride, padding=1)
    assert tuple(h.shape[-2:]) == (c["Ho"], c["Wo"])
    want = (h.half().double() + c["tv"].double()[:, :, None, None] + c["res"].double().permute(0, 3, 1, 2)).half().double().permute(0, 2, 3, 1)
    assert torch.equal(R.conv_ref(c)[0], want)
    hh = h.permute(0, 2, 3, 1)
    assert bool((hh != R.round16(hh)).any()) and bool((hh == R.round16(hh)).any())
    assert len({tuple(r) for r in c["tv"].tolist()}) == B


@pytest.mark.parametrize("shape", R.CONV_CAT_SHAPES)
def test_conv_cat_reference_is_conv2d_plus_the_1x1_shortcut(shape):
    B, H, W, Cin, Cin2, Co = shape
    c = R.conv_case(B, H, W, Cin, Co, Cin2=Cin2)
    want = F.conv2d(c["x"].double().permute(0, 3, 1, 2), c["w"].double(), None, padding=1) + F.conv2d(c["x2"].double().permute(0, 3, 1, 2), c["wsc"].double()[:, :, None, None]) \
        + c["bias"].double()[None, :, None, None]
    assert torch.equal(R.conv_ref(c)[0], want.half().double().permute(0, 2, 3, 1))


@pytest.mark.parametrize("kind,shape", [("in", s) for s in R.CONV_IN_SHAPES] + [("out", s) for s in R.CONV_OUT_SHAPES])
def test_boundary_conv_reference_is_conv2d(kind, shape):
    c = R.boundary_case(kind, *shape)
    want = F.conv2d(c["x"].double().permute(0, 3, 1, 2), c["w"].double(), c["bias"].double(), padding=1).half().double().permute(0, 2, 3, 1)
    assert torch.equal(R.boundary_ref(c)[0], want)


GN_ALL_SHAPES = R.GN_SHAPES + tuple(s[:3] for s in R.GN_STATS_SHAPES)          # every shape a GPU test sends through gn_ref


@pytest.mark.parametrize("shape", GN_ALL_SHAPES)
def test_groupnorm_reference_is_group_norm(shape):
    B, HW, C_ = shape
    for real in (False, True):
        c = R.gn_case(B, HW, C_, real=real)
        for silu, eps in R.GN_VARIANTS[:3]:
            ref, bound, _ = R.gn_ref(c, silu, eps)
            want = F.group_norm(c["x"].double().transpose(1, 2), R.GN_GROUPS, c["gamma"].double(), c["beta"].double(), R.f32(eps))
            _close(ref, (F.silu(want) if silu else want).transpose(1, 2), 1e-9)
            assert bool((bound > 0).all())
            if not real:      # about half an fp16 ulp, not a tolerance
                _tight(bound, ref, 3e-6)


def test_groupnorm_lattice_gives_every_group_its_own_statistics():
    c = R.gn_case(2, 64, 320)
    st = R.gn_stats(c)
    mean = st[..., 0] / (64 * 10)
    assert bool((mean[:, 1:] - mean[:, :-1]).abs().min() > 0.5) and bool((mean[0] - mean[1]).abs().min() > 0.5)


@pytest.mark.parametrize("shape", R.LN_SHAPES)
def test_layernorm_reference_is_layer_norm(shape):
    c = R.ln_case(*shape)
    for eps in (1e-5, 1e-6):
        ref, bound = R.ln_ref(c, eps)
        _close(ref, F.layer_norm(c["x"].double(), (shape[1],), c["gamma"].double(), c["beta"].double(), R.f32(eps)), 1e-9)
        _tight(bound, ref, 1e-5)


@pytest.mark.parametrize("shape,geglu", [(s, False) for s in R.LNFOLD_SHAPES] + [((77, 128, 512), True), ((300, 256, 768), True)])
def test_folded_layernorm_reference_is_layer_norm_then_linear(shape, geglu):
    M, C_, N = shape
    c = R.lnfold_case(M, C_, N, geglu=geglu)
    t, st = R.lnfold_producer(c)
    want_t = (F.linear(c["X"].double(), c["Wp"].double()).half().double() + c["R"].double()).half().double()
    assert torch.equal(t, want_t) and bool((t * 4 == torch.floor(t * 4)).all()), "the producer's outputs must stay on the 1/4 lattice"
    assert torch.equal(st[:, 0], t.sum(1)) and torch.equal(st[:, 1], (t * t).sum(1))
    ratio = (t.mean(1).abs() / t.std(1, unbiased=False))
    assert float((ratio >= 10).double().mean()) >= 0.24, "a quarter of the rows must have |mean| / std of 10 or more"
    h, E = R.lnfold_ref(c, t)
    want = F.linear(F.layer_norm(t, (C_,), c["gamma"].double(), c["beta"].double(), R.f32(c["eps"])), c["W"].double(), c["bias"].double())
    _close(h, want, 1e-9)
    Wf, cs, (lb, lbb) = R.lnfold_weights(c)
    assert torch.equal(Wf, (c["W"].double() * c["gamma"].double()).half().double())
    assert R.lnfold_exactness(c, t) < R.LIMIT
    # fp32 accumulation of the statistics in a scrambled order reproduces fp64
    assert torch.equal(R.scrambled_fp32_sum(t, 1, 8), st[:, 0]) and torch.equal(R.scrambled_fp32_sum(t * t, 2, 8), st[:, 1])
    assert torch.equal(R.scrambled_fp32_sum(Wf, 3, 64), cs)
    # the bound is of the size of the fp32 operations behind the accumulator -- the cancellation on the shifted rows included -- not a tolerance
    assert float((E / (h.abs() + 1.0)).max()) < 2e-4


def test_elementwise_references_against_torch_in_fp64():
    c = R.ew_case(4, 3, 33 * 33)
    B, per = c["B"], c["per"]
    x, eu, ec = (c[k].double().reshape(B, per) for k in ("x", "eu", "ec"))
    co = c["ddim_coef"].double()
    want = co[:, 1:2] * x + co[:, 2:3] * torch.lerp(eu, ec, co[:, 0:1])
    ref, bound = R.ddim_ref(c, c["ddim_coef"])
    _close(ref.reshape(B, per), want)
    _tight(bound, ref, 1e-5)
    bc = c["blend_coef"].double()
    m = c["mask"].double().reshape(B, 1, c["HW"])
    keep = bc[:, 0].reshape(B, 1, 1) * c["init"].double().reshape(B, 3, -1) + bc[:, 1].reshape(B, 1, 1) * c["noise"].double().reshape(B, 3, -1)
    _close(R.blend_ref(c, c["blend_coef"])[0].reshape(B, 3, -1), torch.lerp(keep, c["x"].double().reshape(B, 3, -1), m.expand(B, 3, c["HW"])))
    p = {k: R.f32(v) for k, v in R.PRIOR_SCALARS.items()}
    s = c["s"].double()
    e_u, e_c = (s - p["sqrt_a"] * c["eu"].double()) / p["sqrt_b"], (s - p["sqrt_a"] * c["ec"].double()) / p["sqrt_b"]
    e = torch.lerp(e_u, e_c, torch.tensor(p["g"], dtype=torch.float64))
    want = p["k0"] * (s - p["sqrt_b"] * e) / p["sqrt_a"] + p["k1"] * s + p["sigma"] * c["noise32"].double()
    ref, bound = R.prior_ref(c)
    _close(ref, want)
    assert float((bound / (ref.abs() + 1.0)).max()) < 1e-5


@pytest.mark.parametrize("shape", R.LINEAR_SHAPES)
def test_linear_small_reference_is_linear(shape):
    c = R.linear_case(*shape)
    assert torch.equal(R.linear_ref(c)[0], F.linear(c["A"].double(), c["W"].double(), c["bias"].double()).half().double())
    h = F.linear(c["A"].double(), c["W"].double(), c["bias"].double())
    assert bool((h != R.round16(h)).any()) and bool((h == R.round16(h)).any())


@pytest.mark.parametrize("shape", R.LINEAR_REAL_SHAPES)
def test_linear_small_silu_reference_and_the_share_of_the_exponential(shape):
    c = R.linear_case(*shape, real=True)
    ref, bound, share = R.linear_ref(c, 1, 1)
    _close(ref, F.silu(F.linear(F.silu(c["A"].double()), c["W"].double(), c["bias"].double())))
    assert share <= 0.1, share
    _tight(bound, ref, 1e-4)


# ---- the conditions that make "exact" true -------------------------------------------------------------------------------------------------------------------
def _brute(A, W, seed, rows=48):
    """fp32 accumulation of the products of `rows` rows in a scrambled order"""
    A, W = R.f64(A)[:rows], R.f64(W)
    terms = A[:, None, :] * W[None, :, :]
    t32 = terms.numpy().astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), terms.numpy()), "a product is not an fp32 value"
    assert torch.equal(R.scrambled_fp32_sum(terms, seed), A @ W.t())


@pytest.mark.parametrize("c", ALL_GEMM + [R.geglu_case(*s) for s in R.GEGLU_SHAPES] + [R.linear_case(*s) for s in R.LINEAR_SHAPES], ids=lambda c: f"{c['M']}x{c['N']}x{c['K']}")
def test_gemm_cases_accumulate_exactly_in_any_order(c):
    assert R.exactness(c) < R.LIMIT
    for k in ("A", "W", "bias", "res"):
        if c.get(k) is not None:
            v = R.f64(c[k]) / c["unit"]
            assert bool((v == torch.floor(v)).all()), f"{k} is off the lattice"
    _brute(c["A"], c["W"], 11)


def _im2col(c, rows=48):
    x = R.f64(c["x"])
    if c.get("up"):
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    cols = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1, stride=c.get("stride", 1))          # [B, Ci 9, L]
    cols = cols.transpose(1, 2).reshape(-1, cols.shape[1])
    pick = torch.linspace(0, cols.shape[0] - 1, rows).long()
    return cols[pick], R.f64(c["w"]).reshape(c["Co"], -1), pick


@pytest.mark.parametrize("c", [R.conv_case(*s) for s in R.CONV_SHAPES] + [R.conv_case(s[0], s[1], s[2], s[3], s[5], Cin2=s[4]) for s in R.CONV_CAT_SHAPES]
                         + [R.boundary_case("in", *s) for s in R.CONV_IN_SHAPES] + [R.boundary_case("out", *s) for s in R.CONV_OUT_SHAPES],
                         ids=lambda c: f"{c['B']}x{c['H']}x{c['W']}x{c['Cin']}->{c['Co']}")
def test_conv_cases_accumulate_exactly_in_any_order(c):
    assert R.exactness(c) < R.LIMIT
    cols, w, pick = _im2col(c)
    _brute(cols, w, 12, rows=len(pick))
    assert torch.equal((cols @ w.t()), R.conv3x3_sum(c["x"], c["w"], c.get("stride", 1), c.get("up", 0)).reshape(-1, c["Co"])[pick])


@pytest.mark.parametrize("c", [R.gn_case(*s) for s in R.GN_SHAPES] + [R.ln_case(*s) for s in R.LN_SHAPES], ids=lambda c: str(tuple(c["x"].shape)))
def test_statistics_sums_are_exact_in_any_order(c):
    assert R.stats_exactness(c) < R.LIMIT
    x = R.f64(c["x"])
    if x.dim() == 3:
        B, HW, C_ = x.shape
        x = x.reshape(B, HW, R.GN_GROUPS, -1).permute(0, 2, 1, 3).reshape(B * R.GN_GROUPS, -1)
        st = R.gn_stats(c).reshape(B * R.GN_GROUPS, 2)
    else:
        st = torch.stack([x.sum(1), (x * x).sum(1)], 1)
    assert torch.equal(R.scrambled_fp32_sum(x, 5, 8), st[:, 0]) and torch.equal(R.scrambled_fp32_sum(x * x, 6, 8), st[:, 1])


def test_column_sum_cases_are_exact_over_runs_of_16_rows():
    for B, HW, C_, C0, rows0, rows1 in R.GN_STATS_SHAPES:
        c = R.gn_case(B, HW, C_)
        x = c["x"].reshape(B * HW, C_)
        assert R.colstats_exactness(x, 0.25) < R.LIMIT and R.stats_exactness(c) < R.LIMIT
        st = R.colstats_ref(x, 16)
        runs = R.f64(x).reshape(-1, 16, C_).permute(0, 2, 1)
        assert torch.equal(R.scrambled_fp32_sum(runs, 7, 4), st[..., 0]) and torch.equal(R.scrambled_fp32_sum(runs * runs, 8, 4), st[..., 1])
        assert torch.equal(R.colstats_ref(x, rows0).reshape(B, -1, C_, 2).sum(1)[:, :, 0], R.f64(c["x"]).sum(1))
    producers = [(c, R.gemm_ref(c, "bias")[0]) for c in (R.gemm_gnstats_case(*s) for s in R.GEMM_GNSTATS_SHAPES)]
    for shape in R.CONV_GNSTATS_SHAPES:
        c = R.conv_gnstats_case(*shape)
        ref = R.conv_ref(c)[0]
        want = F.conv2d(c["x"].double().permute(0, 3, 1, 2), c["w"].double(), c["bias"].double(), padding=1).half().double().permute(0, 2, 3, 1)
        assert torch.equal(ref, want)
        producers.append((c, ref.reshape(-1, shape[4])))
    for c, ref in producers:          # the stored outputs of the producers: multiples of 2^-8 whose sums and squares add exactly over a run of 16 rows
        assert R.exactness(c) < R.LIMIT and R.colstats_exactness(ref, R.WUNIT) < R.LIMIT
        runs = ref.reshape(-1, 16, ref.shape[1]).permute(0, 2, 1)
        st = R.colstats_ref(ref, 16)
        assert torch.equal(R.scrambled_fp32_sum(runs, 10, 4), st[..., 0]) and torch.equal(R.scrambled_fp32_sum(runs * runs, 9, 4), st[..., 1])


def test_groupnorm_cases_reach_every_implementation():
    routes = {R.gn_route(*s) for s in R.GN_SHAPES}
    assert {("fused", 5, 2), ("fused", 10, 4), ("fused", 15, 4), ("fused", 5, 6), ("fused", 10, 16), ("twopass", 1), ("twopass", 2)} <= routes, routes
    fused = {s[2] // R.GN_GROUPS for s in R.GN_SHAPES if R.gn_route(*s)[0] == "fused"}
    assert {10, 20, 30, 40, 60, 80} <= fused, fused
    assert any(s[1] == 70 for s in R.GN_SHAPES) and any(s[0] == 5 for s in R.LN_SHAPES)
    assert {R.gn_route(*s)[0] for s in R.GN_REAL_SHAPES} == {"fused", "twopass"}
    assert sorted({(s[1] // 8 + 63) // 64 for s in R.LN_SHAPES}) == [1, 2, 3, 4]


# ---- the cap on the exponential model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GN_ALL_SHAPES)
def test_exponential_model_stays_below_a_tenth_of_every_silu_bound(shape):
    for real in ((False, True) if shape in R.GN_REAL_SHAPES else (False,)):
        c = R.gn_case(*shape, real=real)
        for eps in (1e-5, 1e-6):
            share = R.gn_ref(c, 1, eps)[2]
            assert 0 < share <= 0.1, (shape, real, eps, share)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------------------
def test_mutant_last_k_tile_dropped_for_one_element():
    for c in ALL_GEMM:
        ref, _ = R.gemm_ref(c)
        K = c["K"]
        tail = c["A"][:, K - 64:].double() @ c["W"][:, K - 64:].double().t()
        m, n = (int(i) for i in np.unravel_index(int(tail.abs().argmax()), tail.shape))          # (an element for which that k-tile's products do not cancel)
        acc = c["A"][m].double() @ c["W"][n].double() - tail[m, n]
        mut = ref.clone()
        mut[m, n] = R.round16(R.round16(acc + c["bias"][n].double()) + c["res"][m, n].double())
        assert int((mut != ref).sum()) == 1
        _rejected("last k-tile dropped", mut, ref)


def test_mutant_k_slab_added_twice_on_one_tile():
    for M, N, K, S in R.SPLITK_SHAPES:
        c = R.gemm_case(M, N, K)
        ref, _ = R.gemm_ref(c)
        per = (K // 64 + S - 1) // S * 64
        slab = c["A"][:64, :per].double() @ c["W"][:64, :per].double().t()
        acc = c["A"].double() @ c["W"].double().t()
        acc[:64, :64] += slab
        mut = R.round16(R.round16(acc + c["bias"].double()) + c["res"].double())
        assert int((mut != ref).sum()) > 0 and bool((mut[64:] == ref[64:]).all())
        _rejected("slab added twice", mut, ref)


def test_mutant_bias_of_the_last_column_missing():
    for c in ALL_GEMM:
        ref, _ = R.gemm_ref(c)
        acc, h, h16, s, out = R.gemm_parts(c)
        mut = ref.clone()
        mut[:, -1] = R.round16(R.round16(acc[:, -1]) + c["res"][:, -1].double())
        _rejected("bias of the last column missing", mut, ref)
    c = R.conv_case(*R.CONV_SHAPES[0])
    ref, _ = R.conv_ref(c)
    c2 = dict(c, bias=c["bias"].clone())
    c2["bias"][-1] = 0
    _rejected("conv bias of the last channel missing", R.conv_ref(c2)[0], ref)


def test_mutant_single_rounding_in_place_of_the_two():
    for c in ALL_GEMM:
        ref, _ = R.gemm_ref(c)
        acc, h, h16, s, out = R.gemm_parts(c)
        _rejected("one rounding", R.round16(h + c["res"].double()), ref)
    c = R.conv_case(*R.CONV_SHAPES[3])
    acc = R.conv3x3_sum(c["x"], c["w"])
    _rejected("conv one rounding", R.round16(acc + c["bias"].double() + c["tv"].double()[:, None, None, :] + c["res"].double()), R.conv_ref(c)[0])


def test_mutant_corner_pixel_with_one_tap_missing():
    for shape in (R.CONV_SHAPES[0], R.CONV_SHAPES[3], R.CONV_SHAPES[4]):
        c = R.conv_case(*shape)
        acc = R.conv3x3_sum(c["x"], c["w"])
        ref, _ = R.conv_ref(c, acc=acc)
        H, W = c["H"], c["W"]
        for (y, x, ky, kx) in ((0, 0, 1, 2), (0, W - 1, 2, 0), (H - 1, 0, 0, 1), (H - 1, W - 1, 0, 0), (0, W // 2, 1, 0), (H // 2, 0, 2, 1)):      # the four corners, two edges
            mut, _ = R.conv_ref(c, drop_tap=(c["B"] - 1, y, x, ky, kx), acc=acc)
            assert int((mut != ref).sum()) >= 1 and bool((mut[0 if c["B"] > 1 else slice(0, 0)] == ref[0 if c["B"] > 1 else slice(0, 0)]).all())
            with pytest.raises(AssertionError, match=rf"'b': {c['B'] - 1}, 'y': {y}, 'x': {x}, "):          # the message names the pixel
                R.accept("corner tap", mut, ref, None, R.CONV_AXES)


@pytest.mark.parametrize("shape", [s for s in R.GN_SHAPES if s[1] <= 70])
def test_mutant_channel_counted_into_the_neighbouring_group(shape):
    c = R.gn_case(*shape)
    for silu, eps in R.GN_VARIANTS:
        ref, bound, _ = R.gn_ref(c, silu, eps)
        for gq, d in ((5, 1), (5, -1), (0, 1), (31, -1)) if (silu, eps) == R.GN_VARIANTS[0] else ((7, 1),):
            mut, _, _ = R.gn_ref(c, silu, eps, stats=R.gn_stats(c, shift_channel=(gq, d)))
            _rejected(f"channel of group {gq} counted into {gq + d}", R.round16(mut), ref, bound)


def test_mutant_table_cell_off_by_one_for_one_gate():
    for shape in R.GEGLU_SHAPES:
        c = R.geglu_case(*shape)
        ref, bound = R.geglu_ref(c)
        h = c["A"].double() @ c["W"].double().t() + c["bias"].double()
        v, g = h.chunk(2, dim=-1)
        i, gc = R.lut_cell(g)
        hit = 0
        for target in (-2.0, -1.0, -0.5, 0.75, 1.0, 2.0):          # (beyond |g| = 2.5 a cell is less than an fp16 step of the output)
            cand = ((g - target).abs() < 0.26) & (v.abs() > 0.5)
            if not bool(cand.any()):
                continue
            m, n = (int(t[0]) for t in cand.nonzero(as_tuple=True))
            x0 = (i[m, n] + 1 - 256) / 32          # the next cell's entry, the gate's own fraction
            lut = R.phi(x0) + (gc[m, n] * 32 + 256 - i[m, n]) * (R.phi(x0 + 1 / 32) - R.phi(x0))
            mut = R.round16(ref)
            mut[m, n] = R.round16(v[m, n] * g[m, n] * lut)
            _rejected(f"table cell off by one at gate {float(g[m, n])}", mut, ref, bound)
            hit += 1
        assert hit >= 4


def test_mutant_row_coefficients_taken_from_the_next_row():
    c = R.ew_case(4, 3, 33 * 33)
    ref, bound = R.ddim_ref(c, c["ddim_coef"])
    wrong = c["ddim_coef"].clone()
    wrong[1] = c["ddim_coef"][2]
    _rejected("ddim coefficients of the next row", R.round16(R.ddim_ref(c, wrong)[0]), ref, bound)
    ref, bound = R.blend_ref(c, c["blend_coef"])
    wrong = c["blend_coef"].clone()
    wrong[1] = c["blend_coef"][2]
    _rejected("blend coefficients of the next row", R.round16(R.blend_ref(c, wrong)[0]), ref, bound)
    # the folded LayerNorm: one row normalised with the next row's statistics; one row with a 64-column statistics slot missing
    cf = R.lnfold_case(*R.LNFOLD_SHAPES[0])
    t, st = R.lnfold_producer(cf)
    h, E = R.lnfold_ref(cf, t)
    for row in (2, 3):
        wrong = st.clone()
        wrong[row] = st[row + 1]
        mut = R.round16(h)
        mut[row] = R.round16(R.lnfold_ref(cf, t, wrong)[0][row])
        _rejected("a row folded with the next row's statistics", mut, h, R.with_store16(h, E))
        wrong = st.clone()
        wrong[row] = torch.stack([t[row, :-64].sum(), (t[row, :-64] ** 2).sum()])
        mut = R.round16(h)
        mut[row] = R.round16(R.lnfold_ref(cf, t, wrong)[0][row])
        _rejected("a statistics slot missing", mut, h, R.with_store16(h, E))


def test_accept_takes_the_correctly_rounded_reference_and_refuses_a_nan():
    c = R.geglu_case(*R.GEGLU_SHAPES[0])
    ref, bound = R.geglu_ref(c)
    assert R.accept("rounded reference", R.round16(ref), ref, bound) <= 1.0
    bad = R.round16(ref)
    bad[3, 5] = float("nan")
    with pytest.raises(AssertionError):
        R.accept("nan", bad, ref, bound)
    off = R.round16(ref)
    off[7, 9] += 4 * R.half_ulp16(ref[7, 9].abs() + 1e-3)          # two fp16 steps: one wrong element among 33 000
    _rejected("one element two ulps off", off, ref, bound)


# ---- refusals: none of these reaches a HIP call ------------------------------------------------------------------------------------------------------------
INVALID, SHAPE = 1, 2          # IA2P_ERR_INVALID, IA2P_ERR_SHAPE (include/ia2p.h): the two statuses a host-side check returns; a failed launch would be IA2P_ERR_HIP (6)


def test_entry_points_refuse_on_the_host(lib):
    from instructany2pix_amd import _ffi
    p = C.c_void_p(4096)          # never dereferenced: every call below is refused before a launch
    d = _ffi.ConvGnC()
    d.x0 = d.Wp = d.y = 4096
    d.C0, d.B, d.H, d.W, d.Co = 64, 1, 16, 16, 60
    rows = C.c_int(7)          # (the one argument these entry points write before they check: the slot size, reset to 0)
    r = C.byref(rows)
    calls = [
        (SHAPE, lib.ia2p_gemm(None, p, p, None, None, p, 64, 64, 96, 0)),                       # K % 64
        (SHAPE, lib.ia2p_gemm(None, p, p, None, None, p, 64, 66, 64, 0)),                       # N % 4
        (SHAPE, lib.ia2p_gemm(None, p, p, None, None, p, 64, 64, 64, 1)),                       # GEGLU without bias
        (SHAPE, lib.ia2p_gemm(None, p, p, p, None, p, 64, 80, 64, 1)),                          # GEGLU: N % 32
        (INVALID, lib.ia2p_gemm(None, None, p, None, None, p, 64, 64, 64, 0)),
        (SHAPE, lib.ia2p_gemm_splitk(None, p, p, None, None, p, 64, 64, 128, 3, p)),            # more slices than k-tiles
        (INVALID, lib.ia2p_gemm_splitk(None, p, p, None, None, p, 64, 64, 128, 2, None)),       # no slab
        (SHAPE, lib.ia2p_gemm_ex(None, p, p, None, None, p, 64, 64, 128, 0, None, None, None, 2, None)),
        (INVALID, lib.ia2p_gemm_ex(None, p, p, p, None, p, 64, 64, 128, 1, None, p, None, 1, None)),      # row statistics of a GEGLU output
        (INVALID, lib.ia2p_gemm_gnstats(None, p, p, None, None, p, 256, 64, 64, 0, None, 256, None, r)),  # no statistics buffer
        (SHAPE, lib.ia2p_gemm_gnstats(None, p, p, None, None, p, 256, 68, 64, 0, None, 256, p, r)),       # N % 8
        (SHAPE, lib.ia2p_gemm_gnstats(None, p, p, None, None, p, 250, 64, 64, 0, None, 256, p, r)),       # M % HW
        (INVALID, lib.ia2p_fold_layernorm(None, p, None, p, None, p, p, p, 64, 64)),            # no gamma
        (INVALID, lib.ia2p_fold_layernorm(None, p, p, p, None, p, p, p, 0, 64)),                # N < 1
        (SHAPE, lib.ia2p_conv3x3(None, p, p, None, None, None, p, 1, 8, 8, 48, 64, 1, 0)),      # Cin % 64
        (SHAPE, lib.ia2p_conv3x3(None, p, p, None, None, None, p, 1, 8, 8, 64, 64, 3, 0)),      # stride
        (SHAPE, lib.ia2p_conv3x3_splitk(None, p, p, None, None, None, p, 1, 8, 8, 64, 64, 10, p)),
        (SHAPE, lib.ia2p_conv3x3_cat(None, p, p, p, None, p, 1, 8, 8, 64, 32, 64)),             # Cin2 % 64
        (INVALID, lib.ia2p_conv3x3_gn(None, None, None)),
        (SHAPE, lib.ia2p_conv3x3_gn(None, C.byref(d), r)),                                      # Co % 8
        (INVALID, lib.ia2p_pack_conv3x3(None, p, None, 64, 64)),
        (SHAPE, lib.ia2p_pack_conv3x3(None, p, p, 64, 48)),                                     # Cin % 64
        (INVALID, lib.ia2p_pack_conv_out(None, None, p, 4, 64)),
        (SHAPE, lib.ia2p_conv_in(None, p, p, p, p, p, 1, 8, 4, 4, 64)),                         # Cin * 9 > 64
        (SHAPE, lib.ia2p_conv_out(None, p, p, p, p, 1, 48, 4, 4, 4)),                           # C % 32
        (SHAPE, lib.ia2p_conv_out(None, p, p, p, p, 1, 64, 4, 4, 9)),                           # Co > 8
        (SHAPE, lib.ia2p_groupnorm_silu(None, p, p, p, p, 1, 64, 100, 32, 1e-5, 1, p)),         # C % 8, C % groups
        (INVALID, lib.ia2p_groupnorm_silu(None, p, p, p, p, 1, 64, 320, 32, 1e-5, 1, None)),
        (INVALID, lib.ia2p_gn_colstats(None, p, 64, 64, 16, None)),
        (SHAPE, lib.ia2p_gn_colstats(None, p, 64, 64, 8, p)),                                   # runs of 16 rows
        (SHAPE, lib.ia2p_gn_colstats(None, p, 72, 64, 16, p)),                                  # rows does not divide M
        (INVALID, lib.ia2p_gn_apply_stats(None, None, 64, p, 64, None, 0, None, 0, p, p, p, 1, 64, 32, 1e-5, 1)),
        (INVALID, lib.ia2p_gn_apply_stats(None, p, 64, None, 64, None, 0, None, 0, p, p, p, 1, 64, 32, 1e-5, 1)),      # no statistics
        (SHAPE, lib.ia2p_gn_apply_stats(None, p, 64, p, 48, None, 0, None, 0, p, p, p, 1, 64, 32, 1e-5, 1)),           # slots that do not divide the image
        (SHAPE, lib.ia2p_gn_apply_stats(None, p, 64, p, 64, None, 0, None, 0, p, p, p, 1, 64, 65, 1e-5, 1)),           # more than 64 groups
        (SHAPE, lib.ia2p_layernorm(None, p, p, p, p, 4, 2056, 1e-5)),                           # C > 2048
        (SHAPE, lib.ia2p_layernorm(None, p, p, p, p, 4, 100, 1e-5)),
        (SHAPE, lib.ia2p_linear_small(None, p, p, None, p, 17, 64, 64, 0, 0)),                  # M > 16
        (SHAPE, lib.ia2p_linear_small(None, p, p, None, p, 4, 64, 60, 0, 0)),                   # K % 8
        (INVALID, lib.ia2p_ddim_step(None, None, p, p, 1.0, 1.0, 1.0, p, None, 8)),
        (INVALID, lib.ia2p_ddim_step_v(None, p, p, p, None, p, None, 1, 8)),                    # no coefficients
        (INVALID, lib.ia2p_ddim_step_v(None, p, p, p, p, p, None, 1, 0)),                       # per < 1
        (INVALID, lib.ia2p_mask_blend(None, p, p, p, None, 1.0, 0.0, p, None, 1, 1, 8)),        # no mask
        (SHAPE, lib.ia2p_mask_blend_v(None, p, p, p, p, p, p, None, 0, 1, 8)),                  # B < 1
        (INVALID, lib.ia2p_prior_step(None, p, None, p, None, 1.0, 0.0, 0.5, 1.0, 1.0, 1.0, p, 8)),   # sqrt_a must be positive
        (SHAPE, lib.ia2p_pack_geglu(None, p, p, 48, 64)),                                       # rows % 32
    ]
    for i, (want, got) in enumerate(calls):
        assert got == want, (i, got, want)
    assert rows.value == 0
