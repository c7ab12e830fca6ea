"""The GEMM and 3x3-convolution options that only the encoders, the VAE and the context projection set -- `act` 1 / 2 / 3 (alone, behind a folded LayerNorm, and chained
as csrc/xf_layer.h chains a transformer block), the epilogue scales, operand strides, a column block of a wider output, the row map with its 16-bit edges, `pad_lo = 0` --
launch by launch through `ia2p_gemm_form` / `ia2p_conv3x3_form` against the fp64 references of tests/encoder_gemm_ref.py.

Operands lie on the lattice of unet_ops_ref (test_encoder_gemm_cpu.py asserts the conditions for every case used here): forms without an activation are held to the exact
bits, activations to the formula's own fp32 error plus half an fp16 ulp. Every launch runs twice into NaN-filled outputs between guard regions and must give the same
bits; every element is compared; with ldc > N the columns outside the block stay the NaN they were; operands with lda / ldw > K carry NaN between their rows.
max(err / bound) is printed per test (pytest -s; docs/LOG.md §42 records a run)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_gemm_ref as R  # noqa: E402
from test_unet_ops_gpu import DEV, Out, _d, _ffi, _p, _twice  # noqa: E402

pytestmark = pytest.mark.gpu
IN_LAUNCH, REDUCE_LAUNCH = R.IN_LAUNCH, R.REDUCE_LAUNCH
ROUTES = (("in-launch", IN_LAUNCH), ("reduce launch", REDUCE_LAUNCH))


@pytest.fixture(scope="module")
def L():
    f = _ffi()
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = f.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    yield lib
    lib.ia2p_debug_set_gemm_tile(-1)
    lib.ia2p_debug_set_splitk_inkernel(-1)


def _report(tag, worst):
    print(f"[encoder-gemm] {tag}: max(err / bound) {worst:.4g}")


def _addr(t, off=0):
    return 0 if t is None else t.data_ptr() + 2 * off


class Form:
    """one case on the device: its storage, its output buffer (M rows of ldc elements, NaN) and the record of the launch"""

    def __init__(self, c, aliased=False, slabs=5):
        f = _ffi()
        self.c, self.aliased = c, aliased
        self.A, self.W = _d(c["A_flat"]), None
        self.W = self.A if c["W_flat"] is c["A_flat"] else _d(c["W_flat"])
        self.bias, self.rowvec, self.Rs = _d(c["bias"]), _d(c["rowvec"]), _d(c.get("R_flat"))
        self.o = Out(c["M"] * c["ldc"])
        self.part = torch.empty(slabs * c["M"] * c["N"], dtype=torch.float32, device=DEV)
        assert not aliased or (c["ldr"] == c["ldc"] and c["col0"] == 0)
        self.init = R.logical(c)[2].half() if aliased else None
        d = self.d = f.GemmFormC()
        d.A, d.lda, d.W, d.ldw = _addr(self.A, c["a_off"]), c["lda"], _addr(self.W, c["w_off"]), c["ldw"]
        d.bias, d.C, d.ldc = _addr(self.bias), self.o.ptr.value + 2 * c["col0"], c["ldc"]
        d.residual, d.ldr = (d.C if aliased else _addr(self.Rs)), c["ldr"]
        d.M, d.N, d.K, d.rpb, d.bstride, d.roff = c["M"], c["N"], c["K"], c["rpb"], c["bstride"], c["roff"]
        d.act, d.acc_scale, d.bias_scale = c["act"], c["e_as"], c["e_bs"]
        d.rowvec, d.rowvec_ld, d.rows_per_batch = _addr(self.rowvec), c["N"], c["rows_per_batch"]
        d.partial = self.part.data_ptr()

    def run(self, L, tag, splitk=0):
        """-> the [M, N] block (CPU). Outside the block every element of the buffer is still the NaN it was"""
        f, c = _ffi(), self.c
        self.d.splitk = splitk

        def launch():
            self.part.fill_(float("nan"))          # a slab read before it is written, or never written, poisons the output
            return L.ia2p_gemm_form(f.current_stream(), C.byref(self.d))
        full = _twice(tag, launch, [self.o], init=self.init, partly=(self.o,))[0].reshape(c["M"], c["ldc"])
        block = full[:, c["col0"]:c["col0"] + c["N"]]
        assert bool(torch.isfinite(block.double()).all()), f"{tag}: an output is not finite (or was never written)"
        outside = torch.ones(c["ldc"], dtype=torch.bool)
        outside[c["col0"]:c["col0"] + c["N"]] = False
        nan_bits = torch.full((1,), float("nan"), dtype=torch.float16).view(torch.int16)
        assert bool((full[:, outside].contiguous().view(torch.int16) == nan_bits).all()), f"{tag}: wrote outside columns [{c['col0']}, {c['col0'] + c['N']}) of its rows"
        return block


def _sweep(L, form, ref, bound, tag, tiles, splits=(), split_tiles=(-1, 0, 12)):
    """the case on every tile in `tiles` unsplit, and on `split_tiles` with every K split in `splits` finished both ways -> max(err / bound)"""
    worst = 0.0
    try:
        for tile in tiles:
            L.ia2p_debug_set_gemm_tile(tile)
            t = f"{tag} tile {tile}"
            worst = max(worst, R.accept(t, form.run(L, t), ref, bound, ("m", "n")))
        for route, limit in ROUTES if splits else ():
            L.ia2p_debug_set_splitk_inkernel(limit)
            for tile in split_tiles:
                L.ia2p_debug_set_gemm_tile(tile)
                for sk in splits:
                    t = f"{tag} {route} tile {tile} split {sk}"
                    worst = max(worst, R.accept(t, form.run(L, t, sk), ref, bound, ("m", "n")))
    finally:
        L.ia2p_debug_set_splitk_inkernel(-1)
        L.ia2p_debug_set_gemm_tile(-1)
    return worst


def _epilogue(c, bias, res):
    d = dict(c)
    if not bias:
        d["bias"] = None
    if not res:
        d["R_flat"] = d["res"] = None
    return d


# ---- 1. activations on an exact pre-activation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("M,N,K", R.ACT_SHAPES)
def test_activation_within_the_formula_bound(L, M, N, K, act):
    base = R.act_case(M, N, K, act, bias=True, res=True)
    worst = 0.0
    for bias, res in R.ACT_EPILOGUES:
        c = _epilogue(base, bias, res != "none")
        ref, bound, _ = R.form_ref(c)
        tag = f"act {act} {M}x{N}x{K} bias {bias} {res}"
        splits = R.ACT_SPLITS[K] if (bias and res != "aliased residual") else ()
        worst = max(worst, _sweep(L, Form(c, aliased=res == "aliased residual"), ref, bound, tag, R.ACT_TILES, splits, (-1, 0, 12, 20)))
    if N % 8 == 4:          # the 8-byte form again, into rows of an odd multiple of 4 elements
        c = dict(base, ldc=N + 8)
        ref, bound, _ = R.form_ref(c)
        worst = max(worst, _sweep(L, Form(c), ref, bound, f"act {act} {M}x{N}x{K} ldc {N + 8}", (-1, 0, 4, 12), R.ACT_SPLITS[K], (-1, 4)))
    _report(f"act {act} {M}x{N}x{K}", worst)


# ---- 2. a folded LayerNorm into an activation ------------------------------------------------------------------------------------------------------------------
def _fold(L, W, gamma, beta, bias):
    f = _ffi()
    N, K = W.shape
    Wf = torch.full_like(W, float("nan"))
    cs, lb = torch.full((N,), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    f.check(L.ia2p_fold_layernorm(f.current_stream(), _p(W), _p(gamma), _p(beta), _p(bias), _p(Wf), _p(cs), _p(lb), N, K))
    torch.cuda.synchronize()
    return Wf, cs, lb


def _gemm(L, tag, A, lda, W, ldw, bias, residual, out, N, M, K, act=0, ln=None, stats=None, splitk=0, part=None, init=None):
    """a contiguous launch of ia2p_gemm_form into `out` (an Out of M N elements; residual may be its own pointer) -> (the output on the CPU, the slots it reports)"""
    f = _ffi()
    d = f.GemmFormC()
    slots = C.c_int(-1)
    d.A, d.lda, d.W, d.ldw, d.bias, d.residual, d.ldr, d.C, d.ldc = A, lda, W, ldw, bias, residual, N, out.ptr.value, N
    d.M, d.N, d.K, d.act, d.splitk = M, N, K, act, splitk
    d.ln = C.addressof(ln) if ln is not None else 0
    d.stats_out, d.stats_slots = (stats.data_ptr(), C.addressof(slots)) if stats is not None else (0, 0)
    d.partial = part.data_ptr() if part is not None else 0

    def launch():
        if part is not None:
            part.fill_(float("nan"))
        if stats is not None:
            stats.fill_(float("nan"))
        return L.ia2p_gemm_form(f.current_stream(), C.byref(d))
    got = _twice(tag, launch, [out], init=init)[0].reshape(M, N)
    return got, slots.value


@pytest.mark.parametrize("M,C_,N", R.LN_ACT_SHAPES)
def test_layernorm_fold_into_an_activation(L, M, C_, N):
    f = _ffi()
    c = R.ln_act_case(M, C_, N)
    t_ref, st_ref = R.lnfold_producer(c)
    Wf, cs, lb = _fold(L, _d(c["W"]), _d(c["gamma"]), _d(c["beta"]), _d(c["bias"]))
    X, Wp, Rr = _d(c["X"]), _d(c["Wp"]), _d(c["R"])
    t, o = Out(M * C_), Out(M * N)
    stats = torch.empty((C_ // 64 + 1) * M * 2, dtype=torch.float32, device=DEV)
    part = torch.empty(2 * M * max(N, C_), dtype=torch.float32, device=DEV)
    refs = {act: R.ln_act_ref(c, t_ref, act)[:2] for act in R.ACTS}
    worst = 0.0
    try:
        for psplit, limit in ((0, IN_LAUNCH), (2, IN_LAUNCH), (2, REDUCE_LAUNCH)):          # the producer through the same entry point: its output and its row statistics are exact
            L.ia2p_debug_set_splitk_inkernel(limit)
            tag = f"ln producer {M}x{C_} split {psplit} limit {limit}"
            got_t, slots = _gemm(L, tag, X.data_ptr(), C_, Wp.data_ptr(), C_, 0, Rr.data_ptr(), t, C_, M, C_, stats=stats, splitk=psplit, part=part)
            R.accept(tag, got_t, t_ref, None, ("m", "k"))
            assert slots >= 1, tag
            R.accept(tag + " statistics", stats.view(-1, M, 2)[:slots].double().cpu().sum(0), st_ref, None, ("m", "sum | sum of squares"))
        ln = f.LnFoldC(stats.data_ptr(), slots, cs.data_ptr(), lb.data_ptr(), c["eps"])
        for act in R.ACTS:
            ref, bound = refs[act]
            for route, limit in ROUTES:
                L.ia2p_debug_set_splitk_inkernel(limit)
                for tile in R.ACT_TILES:
                    L.ia2p_debug_set_gemm_tile(tile)
                    for csplit in (0, 2):
                        if limit == REDUCE_LAUNCH and not csplit:
                            continue
                        tag = f"ln + act {act} {M}x{C_}->{N} {route} tile {tile} split {csplit}"
                        got, _ = _gemm(L, tag, t.ptr.value, C_, Wf.data_ptr(), C_, 0, 0, o, N, M, C_, act=act, ln=ln, splitk=csplit, part=part)
                        worst = max(worst, R.accept(tag, got, ref, bound, ("m", "n")))
    finally:
        L.ia2p_debug_set_splitk_inkernel(-1)
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"ln + act {M}x{C_}->{N}", worst)


# ---- 3. one transformer block as csrc/xf_layer.h chains it, on real values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", R.ACTS)
def test_xf_layer_round_launch_by_launch(L, act):
    """QKV with the first LayerNorm folded; out-projection with the residual in place, leaving row statistics; fc1 with the second LayerNorm folded and the activation;
    fc2 with the residual in place, leaving row statistics. Each launch is compared on its own with fp64 from the bits the launch before it stored, and consumes the slot
    count and the statistics that launch reported."""
    f = _ffi()
    c = R.xf_case()
    M, H, I, eps = c["M"], c["H"], c["I"], c["eps"]
    x0, att = c["x"], _d(c["att"])
    fq = _fold(L, _d(c["w_qkv"]), _d(c["ln1_g"]), _d(c["ln1_b"]), _d(c["b_qkv"]))
    f1 = _fold(L, _d(c["w_fc1"]), _d(c["ln2_g"]), _d(c["ln2_b"]), _d(c["b_fc1"]))
    wo, bo, w2, b2 = _d(c["w_o"]), _d(c["b_o"]), _d(c["w_fc2"]), _d(c["b_fc2"])
    x, qkv, ff = Out(M * H), Out(M * 3 * H), Out(M * I)
    st = torch.empty((H // 64 + 1) * M * 2, dtype=torch.float32, device=DEV)
    worst = {}

    def stats_check(tag, x16, slots):
        assert slots >= 1, tag
        want, bound = R.row_stats_ref(x16, None)
        return R.accept(tag + " statistics", st.view(-1, M, 2)[:slots].double().cpu().sum(0), want, bound, ("m", "sum | sum of squares"))

    # the entry state: x and its row statistics, as an embedding launch would leave them (one slot, fp32 sums taken here in fp64 and rounded)
    x.reset(x0)
    s0, _ = R.row_stats_ref(x0, None)
    st.fill_(float("nan"))
    st.view(-1, M, 2)[0].copy_(s0.float())
    slots = 1
    ln = f.LnFoldC(st.data_ptr(), slots, fq[1].data_ptr(), fq[2].data_ptr(), eps)
    got, _ = _gemm(L, "xf qkv", x.ptr.value, H, fq[0].data_ptr(), H, 0, 0, qkv, 3 * H, M, H, ln=ln)
    h, E = R.real_lnfold(x0, fq[0].cpu(), fq[1].cpu(), fq[2].cpu(), eps)
    worst["qkv"] = R.accept("xf qkv", got, h, R.with_store16(h, E), ("m", "n"))
    # out-projection: x = fp16(fp16(att Wo^T + bo) + x), in place
    v, E = R.real_gemm(c["att"], c["w_o"], c["b_o"])
    ref, bound, _ = R.epilogue_ref(v, E, 0, None, R.f64(x0))
    x1, slots = _gemm(L, "xf out-projection", att.data_ptr(), H, wo.data_ptr(), H, bo.data_ptr(), x.ptr.value, x, H, M, H, stats=st, init=x0)
    worst["out-projection"] = R.accept("xf out-projection", x1, ref, bound, ("m", "n"))
    worst["statistics 1"] = stats_check("xf out-projection", x1, slots)
    # fc1: ff = act(LayerNorm(x) W1^T + b1) from the stored x1 and the statistics just written
    ln = f.LnFoldC(st.data_ptr(), slots, f1[1].data_ptr(), f1[2].data_ptr(), eps)
    x.reset(x1)
    got, _ = _gemm(L, "xf fc1", x.ptr.value, H, f1[0].data_ptr(), H, 0, 0, ff, I, M, H, act=act, ln=ln)
    h, E = R.real_lnfold(x1, f1[0].cpu(), f1[1].cpu(), f1[2].cpu(), eps)
    ref, bound, _ = R.epilogue_ref(h, E, act)
    worst["fc1"] = R.accept("xf fc1", got, ref, bound, ("m", "n"))
    # fc2: x = fp16(fp16(ff W2^T + b2) + x), in place
    v, E = R.real_gemm(got, c["w_fc2"], c["b_fc2"])
    ref, bound, _ = R.epilogue_ref(v, E, 0, None, R.f64(x1))
    x2, slots = _gemm(L, "xf fc2", ff.ptr.value, I, w2.data_ptr(), I, b2.data_ptr(), x.ptr.value, x, H, M, I, stats=st, init=x1)
    worst["fc2"] = R.accept("xf fc2", x2, ref, bound, ("m", "n"))
    worst["statistics 2"] = stats_check("xf fc2", x2, slots)
    print(f"[encoder-gemm] xf_layer round act {act}: max(err / bound) " + ", ".join(f"{k} {v:.4g}" for k, v in worst.items()))


# ---- 4. epilogue scales ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", R.SCALE_FORMS, ids=lambda s: s[0])
@pytest.mark.parametrize("M,N,K,rpbatch", R.SCALE_SHAPES)
def test_epilogue_scales_are_fp64_to_the_bit(L, M, N, K, rpbatch, form):
    c = R.scale_case(M, N, K, rpbatch, form)
    ref, bound, _ = R.form_ref(c)
    assert bound is None
    _report(c["tag"], _sweep(L, Form(c), ref, None, c["tag"], R.SCALE_TILES, (2,), (-1, 0, 12)))


def test_power_of_two_scales_commute_with_scaling_the_inputs(L):
    """acc_scale = bias_scale = 2^-3 gives the bits of the same launch with A, the bias and the row vector scaled on the host (the residual is not scaled)"""
    M, N, K, rpbatch = R.SCALE_SHAPES[0]
    c = R.scale_case(M, N, K, rpbatch, R.SCALE_FORMS[0])
    A, W, _ = R.logical(c)
    pre = dict(c, e_as=1.0, e_bs=1.0, A_flat=(A * 0.125).half().reshape(-1), bias=(R.f64(c["bias"]) * 0.125).half(), rowvec=(R.f64(c["rowvec"]) * 0.125).half())
    assert torch.equal(R.f64(pre["bias"]) * 8, R.f64(c["bias"])) and torch.equal(R.f64(pre["rowvec"]) * 8, R.f64(c["rowvec"]))
    for tile in (-1, 0, 12):
        L.ia2p_debug_set_gemm_tile(tile)
        try:
            a, b = Form(c).run(L, f"scaled in the epilogue tile {tile}"), Form(pre).run(L, f"scaled on the host tile {tile}")
        finally:
            L.ia2p_debug_set_gemm_tile(-1)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"tile {tile}: scaling in the epilogue and scaling the inputs give other bits"
    _report("power-of-two scales commute", 0.0)


# ---- 5. strides and the row map -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.stride_cases()))
def test_operand_and_output_strides_are_fp64_to_the_bit(L, name):
    c = R.stride_cases()[name]
    ref, bound, _ = R.form_ref(c)
    assert bound is None
    _report(name, _sweep(L, Form(c), ref, None, name, (-1, 0, 4, 12, 20), (2,) if c["K"] >= 128 else (), (-1, 0)))


@pytest.mark.parametrize("name", list(R.ROWMAP_SHAPES))
def test_row_map_is_fp64_to_the_bit(L, name):
    c = R.rowmap_case(name)
    ref, bound, _ = R.form_ref(c)
    assert bound is None
    big = c["M"] > 1000
    _report(name, _sweep(L, Form(c, slabs=1 if big else 2), ref, None, name, (-1, 12) if big else (-1, 0, 4, 12, 20), () if big or c["K"] < 128 else (2,), (-1, 0)))


# ---- 6. the 3x3 convolution: pad_lo, the upsampled view and the scales -------------------------------------------------------------------------------------------
def _pack3(L, w):
    f = _ffi()
    Co, Cin = w.shape[:2]
    wp = torch.full((Co, 9 * Cin), float("nan"), dtype=torch.half, device=DEV)
    f.check(L.ia2p_pack_conv3x3(f.current_stream(), _p(w), _p(wp), Co, Cin))
    torch.cuda.synchronize()
    return wp


def _conv_sweep(L, c, tag, tiles, split_tiles):
    f = _ffi()
    ref, bound = R.conv_form_ref(c)
    assert bound is None
    x, b, tv, res = _d(c["x"]), _d(c["bias"]), _d(c["tv"]), _d(c["res"])
    wp = _pack3(L, _d(c["w"]))
    o = Out(ref.numel())
    part = torch.empty(3 * ref.numel(), dtype=torch.float32, device=DEV)
    d = f.ConvFormC()
    d.x, d.Wp, d.bias, d.rowvec, d.residual, d.y = x.data_ptr(), wp.data_ptr(), b.data_ptr(), _addr(tv), _addr(res), o.ptr.value
    d.B, d.Hs, d.Ws, d.Cin, d.Co, d.stride, d.up, d.pad_lo = c["B"], c["H"], c["W"], c["Cin"], c["Co"], c["stride"], c["up"], c["pad_lo"]
    d.acc_scale, d.bias_scale, d.partial = c["e_as"], c["e_bs"], part.data_ptr()

    def launch():
        part.fill_(float("nan"))
        return L.ia2p_conv3x3_form(f.current_stream(), C.byref(d))
    try:
        for tile in tiles:
            L.ia2p_debug_set_gemm_tile(tile)
            d.splitk = 0
            t = f"{tag} tile {tile}"
            R.accept(t, _twice(t, launch, [o])[0], ref, None, R.CONV_AXES)
        for route, limit in ROUTES:
            L.ia2p_debug_set_splitk_inkernel(limit)
            for tile in split_tiles:
                L.ia2p_debug_set_gemm_tile(tile)
                for sk in (1, 2, 3):
                    d.splitk = sk
                    t = f"{tag} {route} tile {tile} split {sk}"
                    R.accept(t, _twice(t, launch, [o])[0], ref, None, R.CONV_AXES)
    finally:
        L.ia2p_debug_set_splitk_inkernel(-1)
        L.ia2p_debug_set_gemm_tile(-1)
    _report(tag, 0.0)


@pytest.mark.parametrize("B,H,W,Cin,Co", R.CONV_PAD0)
def test_conv3x3_stride_2_without_the_leading_pad_is_fp64_to_the_bit(L, B, H, W, Cin, Co):
    c = R.conv_form_case(B, H, W, Cin, Co, stride=2, pad_lo=0, e_bs=0.25)
    _conv_sweep(L, c, f"conv3x3 pad_lo 0 stride 2 {(B, H, W, Cin, Co)}", (-1, 0, 4, 12, 18, 20, 24), (-1, 0, 12))


def test_conv3x3_upsampled_with_a_scaled_bias_is_fp64_to_the_bit(L):
    c = R.conv_form_case(*R.CONV_UP, up=1, e_bs=0.25)
    _conv_sweep(L, c, f"conv3x3 up 1 bias_scale 2^-2 {R.CONV_UP}", (-1, 0, 4, 12, 20, 24, 25, 26), (-1, 0, 24))


def test_conv3x3_scaled_with_a_residual_is_fp64_to_the_bit(L):
    c = R.conv_form_case(*R.CONV_SCALED, e_as=0.125, e_bs=0.125)
    _conv_sweep(L, c, f"conv3x3 acc_scale = bias_scale = 2^-3 {R.CONV_SCALED}", (-1, 0, 8, 12, 18, 24, 25, 26), (-1, 0, 12, 24, 25, 26))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(L):
    """everything the two entry points refuse (the lists of encoder_gemm_ref, also walked without a GPU): the stated status, and not one element of the output, the
    statistics or the slabs written. (The fused attention entry points have no field for an activation or a row map: there is nothing to refuse there.)"""
    f = _ffi()
    bufs = {}

    def ptr(name):
        if name not in bufs:
            bufs[name] = torch.full((1 << 16,), float("nan"), dtype=torch.float16, device=DEV)
        return bufs[name].data_ptr()
    for kind, todo, fn in (("gemm", R.GEMM_REFUSALS, L.ia2p_gemm_form), ("conv", R.CONV_REFUSALS, L.ia2p_conv3x3_form)):
        assert fn(f.current_stream(), None) == R.INVALID
        for what, changes, status in todo:
            d, keep = R.refusal_record(kind, f, ptr, changes)
            slots = C.c_int(7)
            if kind == "gemm":
                d.stats_slots = C.addressof(slots)
            got = fn(f.current_stream(), C.byref(d))
            assert got == status, (kind, what, got, status)
            assert kind != "gemm" or slots.value == 0, (what, "the slot count is reset before the checks")
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert bool(torch.isnan(b).all()), f"a refused call wrote to {name}"
    _report(f"{len(R.GEMM_REFUSALS) + len(R.CONV_REFUSALS) + 2} refusals", 0.0)
