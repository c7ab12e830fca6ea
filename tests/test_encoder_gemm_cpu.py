"""What tests/test_encoder_gemm_gpu.py rests on, checked without a GPU: the lattice and `exactness` conditions of every case the GPU file uses (the case lists are the
reference module's); the coverage condition on the pre-activations; the cap on the modelled terms (hardware reciprocal, native exponential, the library's tanhf: a
tenth of every bound, with the one exception encoder_gemm_ref's docstring states); the references against a brute-force fp32 evaluation over scrambled chunks with the
kernels' formulas in numpy fp32 -- which is also the CPU measurement of each formula's error; PLANTED FAULTS, each of which `accept`, the comparison the GPU tests
call, must refuse at a named case; and the faults no fp16 comparison can see, listed with the reason. pytest -s prints max(err / bound) for each (docs/LOG.md §42)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_gemm_ref as R  # noqa: E402

LIMIT = 2.0 ** 24


def _say(tag, n):
    print(f"[encoder-gemm cpu] {tag}: max(err / bound) {n:.4g}")


def _ratio(got, ref, bound):
    return R.worst(got, ref, bound)[1]


def _refused(tag, mutant, ref, bound):
    """the reference passes, the mutant (stored as fp16, as a kernel would) is refused -> max(err / bound) of the mutant (the number of differing elements if exact)"""
    R.accept(tag + " (the reference itself)", R.round16(ref), ref, bound)
    got = R.round16(mutant)
    with pytest.raises(AssertionError, match="worst at"):
        R.accept(tag, got, R.round16(ref) if bound is None else ref, bound)
    n = _ratio(got, R.round16(ref) if bound is None else ref, bound)
    _say("planted: " + tag, n)
    return n


def _act_cases():
    for s in R.ACT_SHAPES:
        for act in R.ACTS:
            for bias, res in R.ACT_EPILOGUES:
                yield R.act_case(*s, act, bias=bias, res=res != "none")


def _all_gemm_cases():
    for s in R.ACT_SHAPES:
        for bias in (True, False):
            yield R.act_case(*s, 1, bias=bias, res=True)
    for s in R.SCALE_SHAPES:
        for form in R.SCALE_FORMS:
            yield R.scale_case(*s, form)
    yield from R.stride_cases().values()
    for name in R.ROWMAP_SHAPES:
        yield R.rowmap_case(name)


def _conv_cases():
    for s in R.CONV_PAD0:
        yield R.conv_form_case(*s, stride=2, pad_lo=0, e_bs=0.25)
    yield R.conv_form_case(*R.CONV_UP, up=1, e_bs=0.25)
    yield R.conv_form_case(*R.CONV_SCALED, e_as=0.125, e_bs=0.125)


# ---- the conditions under which "exact" is true -----------------------------------------------------------------------------------------------------------------
def test_every_gemm_case_is_on_the_lattice():
    for c in _all_gemm_cases():
        assert R.exactness(c) < LIMIT, c["tag"]
        v, exact = R.pre_activation(c)
        pow2 = all(math_is_pow2(s) for s in (c["e_as"], c["e_bs"]))
        if pow2:
            assert exact, (c["tag"], "power-of-two scales: no fp32 step may round")
        else:          # the one correctly rounded product: no bias behind it, the accumulator exact
            assert c["bias"] is None and c["rowvec"] is None and c["res"] is None, c["tag"]
        A, W, _ = R.logical(c)
        assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(W).all()), c["tag"]
        # whatever the launch must not read is NaN: a stride of the wrong size finds it
        if c["lda"] > c["K"] and c["A_flat"] is not c["W_flat"]:
            assert bool(torch.isnan(c["A_flat"]).any()), c["tag"]
        if c["ldw"] > c["K"] and c["A_flat"] is not c["W_flat"]:
            assert bool(torch.isnan(c["W_flat"]).any()), c["tag"]


def math_is_pow2(s):
    m, _ = np.frexp(float(s))
    return m == 0.5


def test_every_conv_case_is_on_the_lattice():
    for c in _conv_cases():
        assert R.conv_form_exactness(c) < LIMIT
        assert math_is_pow2(c["e_as"]) and math_is_pow2(c["e_bs"])
    # the sizes were chosen for the pad behind the image: 10 x 14 reads it in its last output row and column, 9 x 7 does not (its last window ends on the image)
    c = R.conv_form_case(*R.CONV_PAD0[0], stride=2, pad_lo=0, e_bs=0.25)
    assert (c["Ho"] - 1) * 2 + 2 == c["H"] and (c["Wo"] - 1) * 2 + 2 == c["W"]
    c = R.conv_form_case(*R.CONV_PAD0[1], stride=2, pad_lo=0, e_bs=0.25)
    assert (c["Ho"] - 1) * 2 + 2 == c["H"] - 1 and (c["Wo"] - 1) * 2 + 2 == c["W"] - 1


def test_ln_act_cases_keep_the_lattice_of_the_folded_layernorm():
    from unet_ops_ref import lnfold_exactness
    for s in R.LN_ACT_SHAPES:
        c = R.ln_act_case(*s)
        t, _ = R.lnfold_producer(c)
        assert lnfold_exactness(c, t) < LIMIT
        far = (t.mean(1).abs() / t.std(1)) > 9.0
        assert 0.2 < float(far.double().mean()) < 0.3, "a quarter of the rows far from zero"


# ---- coverage of the pre-activations ------------------------------------------------------------------------------------------------------------------------------
def test_pre_activation_coverage():
    for s in R.ACT_SHAPES:
        for bias in (True, False):
            c = R.act_case(*s, 1, bias=bias)
            v, exact = R.pre_activation(c)
            assert exact
            lo, hi = R.coverage(v)
            assert lo >= 0.25 and hi >= 0.25, (c["tag"], bias, lo, hi)
            if bias:
                b = R.f64(c["bias"])
                assert [float(b[j]) for j in (0, 2, 3, 5)] == [12.0, -12.0, 60.0, -60.0]
                third = b[1::3]
                assert bool(((third >= 48) & (third < 64)).all())
                assert float((v - b).abs().max()) < 28.0          # the sums themselves: the +-60 columns stay beyond +-32
                assert float(v[:, 3].min()) > 32 and float(v[:, 5].max()) < -32 and float(v[:, 5].min()) * -R.C_QUICK > 88.8, "quick-GELU's __expf must overflow somewhere"
                others = torch.ones(c["N"], dtype=torch.bool)
                others[1::3] = False
                others[[0, 2, 3, 5]] = False
                assert len(set(b[others].tolist())) == int(others.sum()), "every column its own bias"
                # pre-activations that are no fp16 values (an activation after an fp16 rounding is another result)
                inside = (v.abs() > 1) & (v.abs() < 8)
                assert float((R.round16(v) != v)[inside].double().mean()) > 0.5
    for s in R.LN_ACT_SHAPES:
        c = R.ln_act_case(*s)
        t, _ = R.lnfold_producer(c)
        h, _ = R.lnfold_ref(c, t)
        lo, hi = R.coverage(h)
        assert lo >= 0.25 and hi >= 0.25, (s, lo, hi)
        assert float(h[:, 3].min()) > 32 and float(h[:, 5].max()) < -32


# ---- the modelled terms: at most a tenth -----------------------------------------------------------------------------------------------------------------------
def test_modelled_share_is_at_most_a_tenth():
    worst = {1: 0.0, 2: 0.0, 3: 0.0, "3 tail": 0.0}
    for c in _act_cases():
        v, _ = R.pre_activation(c)
        _, bound, share = R.form_ref(c)
        assert bool((bound > 0).all())
        if c["act"] == 3:
            keep = v >= R.TANH_TENTH_FROM
            worst["3 tail"] = max(worst["3 tail"], float(share[~keep].max()))
            # below: the bound IS the model (docstring "the tenth"): at most 0.5 |v| 2^-22 and the counted terms, 8e-7 in absolute terms up to |v| = 6.5
            tail = ~keep & (v >= -6.5)
            if c["res"] is None:
                assert float(bound[tail].max()) < 8e-7 + 2.0 ** -11 * float(R.act64(v, 3)[tail].abs().max())
            share = share[keep]
        worst[c["act"]] = max(worst[c["act"]], float(share.max()))
    for s in R.LN_ACT_SHAPES:
        c = R.ln_act_case(*s)
        t, _ = R.lnfold_producer(c)
        for act in R.ACTS:
            _, bound, share, h = R.ln_act_ref(c, t, act)
            worst[act] = max(worst[act], float((share[h >= R.TANH_TENTH_FROM] if act == 3 else share).max()))
    print(f"[encoder-gemm cpu] modelled share of the bound: {worst}")
    assert worst[1] <= 0.1 and worst[2] <= 0.1 and worst[3] <= 0.1, worst
    assert worst["3 tail"] > 0.5, "the exception is stated because the tail needs it"


# ---- the formulas in numpy fp32 against fp64, over every pre-activation the cases use ------------------------------------------------------------------------------
def _every_pre_activation():
    vs = []
    for s in R.ACT_SHAPES:
        for bias in (True, False):
            vs.append(R.pre_activation(R.act_case(*s, 1, bias=bias))[0].reshape(-1))
    for s in R.LN_ACT_SHAPES:
        c = R.ln_act_case(*s)
        vs.append(R.round32(R.lnfold_ref(c, R.lnfold_producer(c)[0])[0]).reshape(-1))
    return torch.unique(torch.cat(vs))


def test_formula_errors_measured_in_fp32():
    v = _every_pre_activation()
    z = v.numpy().astype(np.float32) * np.float32(0.70710678118654752440)
    erf_err = float(np.abs(R.erf_poly32(z).astype(np.float64) - torch.special.erf(torch.from_numpy(z.astype(np.float64))).numpy()).max())
    print(f"[encoder-gemm cpu] {v.numel()} distinct pre-activations in [{float(v.min()):.4g}, {float(v.max()):.4g}]; |erf_poly32 - erf| <= {erf_err:.3g} (GELU_ERF_CPU {R.GELU_ERF_CPU})")
    assert erf_err <= R.GELU_ERF_CPU
    for act in R.ACTS:
        ref, B, M = R.act_bound(v, act)
        err = (R.act32(v, act) - ref).abs()
        counted = B - R.SECOND * M          # numpy's division, exp and tanh are not the device's: held to the counted part plus ONE ulp of each (half the model)
        r_full = float(torch.where(err == 0, err, err / B).max())
        r_counted = float(torch.where(err == 0, err, err / (counted + 0.5 * M)).max())
        print(f"[encoder-gemm cpu] act {act} in numpy fp32 against fp64: max |err| {float(err.max()):.3g}, max(err / fp32 bound) {r_full:.3g}, against the counted terms and half the model {r_counted:.3g}")
        assert r_full <= 1.0 and r_counted <= 1.0, (act, r_full, r_counted)
        assert bool((R.act32(v, act)[v < -60 / 1.0001] == 0).all()) if act == 2 else True


# ---- the reference against a brute-force fp32 evaluation -----------------------------------------------------------------------------------------------------------
def _brute(c, seed):
    """steps 1 .. 7 in numpy fp32 on an accumulator summed in scrambled fp32 chunks"""
    f = np.float32
    A, W, Rr = R.logical(c)
    acc = R.scrambled_fp32_sum(A[:, None, :] * W[None, :, :], seed)
    assert torch.equal(acc, A @ W.t()), "the lattice makes every summation order exact"
    v = (acc.numpy().astype(f) * f(c["e_as"])).astype(f)
    if c["bias"] is not None:
        v = (R.f64(c["bias"]).numpy() * float(c["e_bs"]) + v.astype(np.float64)).astype(f)
    v = R.act32(torch.from_numpy(v.astype(np.float64)), c["act"]).numpy().astype(f)
    if c["rowvec"] is not None or Rr is not None:
        v = v.astype(np.float16).astype(f)
    if c["rowvec"] is not None:
        rv = R.f64(c["rowvec"])[torch.arange(c["M"]) // c["rows_per_batch"]].numpy()
        v = (rv * float(c["e_bs"]) + v.astype(np.float64)).astype(f)
    if Rr is not None:
        v = (v + Rr.numpy().astype(f)).astype(f)
    return torch.from_numpy(v.astype(np.float16).astype(np.float64))


def test_reference_reproduces_a_brute_force_fp32_evaluation():
    cases = [R.act_case(*R.ACT_SHAPES[i], act, bias=b, res=r) for i in (0, 1) for act in R.ACTS for b, r in ((True, True), (False, False), (True, False))]
    cases += [R.scale_case(*R.SCALE_SHAPES[0], form) for form in R.SCALE_FORMS]
    cases += [c for c in R.stride_cases().values()] + [R.rowmap_case(n) for n in list(R.ROWMAP_SHAPES)[:4]]
    worst = 0.0
    for i, c in enumerate(cases):
        ref, bound, _ = R.form_ref(c)
        worst = max(worst, R.accept(f"brute force {c['tag']}", _brute(c, 100 + i), ref, bound, ("m", "n")))
    _say("brute-force fp32 evaluation of every form", worst)


def test_conv_reference_is_conv2d_on_the_padded_image():
    import torch.nn.functional as F
    for c in _conv_cases():
        x = c["x"].double().permute(0, 3, 1, 2)
        if c["up"]:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        x = F.pad(x, (c["pad_lo"], 1, c["pad_lo"], 1))
        acc = F.conv2d(x, c["w"].double(), None, stride=c["stride"]).permute(0, 2, 3, 1)
        assert torch.equal(acc, R.conv_form_sum(c["x"], c["w"], c["stride"], c["up"], c["pad_lo"]))
        h = (acc * c["e_as"] + c["bias"].double() * c["e_bs"]).half().double()
        want = (h + c["tv"].double()[:, None, None, :] * c["e_bs"] + c["res"].double()).half().double()
        assert torch.equal(R.conv_form_ref(c)[0], want)
        assert bool((acc * c["e_as"] + c["bias"].double() * c["e_bs"] != h).any()), "some outputs must need the first rounding"


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------------------------------
BIG = (130, 200, 640)


def test_planted_activation_faults_are_refused():
    for act, other in ((1, 3), (3, 1)):
        c = R.act_case(*BIG, act)
        v, _ = R.pre_activation(c)
        ref, bound, _ = R.form_ref(c)
        mutant = R.form_ref(c, fault="act 1 <-> 3")[0]
        _refused(f"act {act} evaluated as act {other} at {c['tag']}", mutant, ref, bound)
        # the two halves of the same case: the negative pre-activations alone refuse it
        neg, pos = (v < 0) & (v > -8), (v > 0)
        n_neg = _ratio(R.round16(mutant)[neg], ref[neg], bound[neg])
        n_pos = _ratio(R.round16(mutant)[pos], ref[pos], bound[pos])
        print(f"[encoder-gemm cpu] act {act} as {other}: max(err / bound) {n_neg:.4g} over the negative pre-activations, {n_pos:.4g} over the positive ones")
        assert n_neg > 100.0
        assert n_pos < 2.5, "positive pre-activations hide the swap (HIDDEN below)"
    c = R.act_case(*BIG, 2)
    v, _ = R.pre_activation(c)
    ref, bound, _ = R.form_ref(c)
    mutant = R.form_ref(c, fault="1.7 for 1.702")[0]
    _refused(f"1.7 for 1.702 at {c['tag']}", mutant, ref, bound)
    neg, pos = (v < 0) & (v > -8), (v > 0)
    n_neg, n_pos = _ratio(R.round16(mutant)[neg], ref[neg], bound[neg]), _ratio(R.round16(mutant)[pos], ref[pos], bound[pos])
    print(f"[encoder-gemm cpu] 1.7 for 1.702: max(err / bound) {n_neg:.4g} over the negative pre-activations, {n_pos:.4g} over the positive ones")
    assert n_neg > 10.0 and n_pos < 3.0
    for act in R.ACTS:
        c = R.act_case(*BIG, act)
        ref, bound, _ = R.form_ref(c)
        _refused(f"act {act} applied after the fp16 rounding at {c['tag']}", R.form_ref(c, fault="act after the fp16 rounding")[0], ref, bound)
        c = R.act_case(*BIG, act, res=True)
        ref, bound, _ = R.form_ref(c)
        _refused(f"act {act} applied after the residual at {c['tag']}", R.form_ref(c, fault="act after the residual")[0], ref, bound)
        c = R.act_case(77, 132, 128, act)
        v, _ = R.pre_activation(c)
        ref, bound, _ = R.form_ref(c)
        mutant = ref.clone()
        mutant[:, -4:] = v[:, -4:]
        _refused(f"act {act} skipped on the last 4 columns at {c['tag']}", mutant, ref, bound)


def test_planted_scale_faults_are_refused():
    both = R.scale_case(*R.SCALE_SHAPES[0], R.SCALE_FORMS[0])
    ref, bound, _ = R.form_ref(both)
    assert bound is None
    _refused(f"the residual scaled by bias_scale at {both['tag']}", R.form_ref(both, fault="residual scaled")[0], ref, None)
    _refused(f"the row vector unscaled at {both['tag']}", R.form_ref(both, fault="rowvec unscaled")[0], ref, None)
    alone = R.scale_case(*R.SCALE_SHAPES[0], R.SCALE_FORMS[1])
    ref, bound, _ = R.form_ref(alone)
    _refused(f"acc_scale applied after the bias at {alone['tag']}", R.form_ref(alone, fault="acc_scale after the bias")[0], ref, None)
    # a product rounded to fp16 steps instead of fp32 ones is another result: the non-power-of-two scale is held to the bit
    sc = R.scale_case(*R.SCALE_SHAPES[0], R.SCALE_FORMS[2])
    ref, _, _ = R.form_ref(sc)
    A, W, _ = R.logical(sc)
    _refused(f"1 / sqrt(512) taken in fp64 instead of fp32 at {sc['tag']}", (A @ W.t()) * 512.0 ** -0.5 * (1 + 2.0 ** -11), ref, None)


def test_planted_addressing_faults_are_refused():
    cases = R.stride_cases()
    c = cases["scores: A and W the halves of one [M, 2 K] tensor"]
    ref, bound, _ = R.form_ref(c)
    _refused("ldw read as K at the score launch", R.form_ref(c, ldw=c["K"])[0], ref, bound)
    c = R.rowmap_case("image-token rows (4, 81, 77)")
    ref, bound, _ = R.form_ref(c)
    _refused("roff off by one at the image-token rows", R.form_ref(c, roff=78)[0], ref, bound)
    c = R.rowmap_case("text rows (77, 81, 0)")
    ref, bound, _ = R.form_ref(c)
    _refused("bstride read as rpb at the text rows", R.form_ref(c, bstride=77)[0], ref, bound)
    c = cases["ldc = 3 N + 8, col0 = N"]
    ref, bound, _ = R.form_ref(c)
    store = torch.full((c["M"], c["ldc"]), float("nan"), dtype=torch.float64)
    store[:, :c["N"]] = ref                      # the block lands at column 0
    _refused("the column offset dropped from C at ldc = 3 N + 8", store[:, c["col0"]:c["col0"] + c["N"]], ref, bound)


def test_planted_convolution_faults_are_refused():
    c = R.conv_form_case(*R.CONV_PAD0[0], stride=2, pad_lo=0, e_bs=0.25)
    ref, bound = R.conv_form_ref(c)
    assert bound is None
    _refused(f"pad_lo = 1 for 0 at {R.CONV_PAD0[0]}", R.conv_form_ref(c, pad_lo=1)[0], ref, None)
    _refused(f"the pad row behind the image missing at {R.CONV_PAD0[0]}", R.conv_form_ref(c, trailing="edge")[0], ref, None)
    s = R.conv_form_case(*R.CONV_SCALED, e_as=0.125, e_bs=0.125)
    ref, _ = R.conv_form_ref(s)
    _refused(f"the residual scaled by bias_scale at {R.CONV_SCALED}", R.conv_form_ref(s, fault="residual scaled")[0], ref, None)
    with pytest.raises(AssertionError, match=r"worst at \{'b': 0, 'y': 3, 'x': 5, 'co': 7\}"):          # the message names b, y, x, co
        bad = ref.clone()
        bad[0, 3, 5, 7] += 1.0
        R.accept("conv axes", bad, ref, None, R.CONV_AXES)


def test_two_fp16_steps_and_a_nan_are_refused():
    for act in R.ACTS:
        c = R.act_case(*BIG, act, res=True)
        ref, bound, _ = R.form_ref(c)
        got = R.round16(ref).half()
        assert R.accept("the rounded reference", got, ref, bound) <= 1.0
        for at in ((0, 0), (65, 100), (129, 199), (7, 5)):
            bits = got.clone().view(torch.int16)
            bits[at] += 2
            _refused(f"act {act}: element {at} two fp16 steps off", bits.view(torch.float16).double(), ref, bound)
        nan = got.double().clone()
        nan[3, 5] = float("nan")
        with pytest.raises(AssertionError, match="worst at"):
            R.accept("a NaN", nan, ref, bound)


HIDDEN = (
    ("act 1 <-> 3 on positive pre-activations", "tanh-GELU and erf-GELU differ by about one fp16 step of the output at most for every x > 0 (at most 1.8 bounds on this lattice, "
     "against 146 and 389 over the negative half of the same case, which is what refuses the swap)"),
    ("1.7 for 1.702 on positive pre-activations", "x sigmoid(1.7 x) and x sigmoid(1.702 x) differ by about one fp16 step at most for x > 0 (2.2 bounds against 52 over the negative half)"),
    ("A&S coefficient 0.3275911 off in its last digit", "it moves GELU by far less than the polynomial's own 1.5e-7 (the figure is printed): no fp16 output moves beyond its bound"),
    ("an activation after the fp16 rounding where the pre-activation is an fp16 value", "the two orders are the same operation there: every third column (bias in [48, 64)) and |v| >= 8"),
)


def test_hidden_faults_are_hidden_for_the_stated_reason():
    c = R.act_case(*BIG, 1)
    v, _ = R.pre_activation(c)
    ref, bound, _ = R.form_ref(c)
    mutant = R.form_ref(c, fault="A&S coefficient")[0]
    n = R.accept("A&S coefficient off in its last digit", R.round16(mutant), ref, bound)
    d = float((mutant - _as_exact(v)).abs().max())
    print(f"[encoder-gemm cpu] hidden: A&S coefficient off in its last digit: max(err / bound) {n:.4g}; the formula moves by {d:.3g}")
    assert d < 2e-7
    assert n <= 1.0 and float((R.round16(mutant) != R.round16(_as_exact(v))).double().mean()) < 0.01
    fp16_v = R.round16(v) == v
    late = R.form_ref(c, fault="act after the fp16 rounding")[0]
    assert torch.equal(late[fp16_v], ref[fp16_v])
    assert len(HIDDEN) == 4


def _as_exact(v):
    """the Abramowitz-Stegun GELU with the right coefficient, in fp64 (what the last-digit mutant is compared with bit by bit)"""
    z = (R.f64(v) / R.SQRT2).abs()
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return 0.5 * R.f64(v) * (1.0 + torch.sign(R.f64(v)) * (1.0 - poly * torch.exp(-z * z)))


# ---- refusals: none of these reaches a HIP call (the GPU file walks the same lists with real buffers and checks that nothing was written) ------------------------------
def test_the_two_entry_points_refuse_on_the_host():
    import ctypes as C
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    lib = _ffi.lib()
    names = {}

    def ptr(name):          # distinct 1 MiB-aligned addresses, never dereferenced
        return names.setdefault(name, (len(names) + 1) << 20)
    for kind, todo, fn in (("gemm", R.GEMM_REFUSALS, lib.ia2p_gemm_form), ("conv", R.CONV_REFUSALS, lib.ia2p_conv3x3_form)):
        assert fn(None, None) == R.INVALID
        assert len({what for what, _, _ in todo}) == len(todo)
        for what, changes, status in todo:
            d, keep = R.refusal_record(kind, _ffi, ptr, changes)
            assert fn(None, C.byref(d)) == status, (kind, what)
            msg = lib.ia2p_last_error(None)
            assert msg and (b"gemm_form" in msg or b"conv3x3_form" in msg), (kind, what, msg)
    # what the refusals must not take with them: the 16-bit edges of the row map pack
    assert {c[1] for c in R.ROWMAP_SHAPES.values()} >= {(2, 3, 65535), (65535, 65536, 1)}
