"""The UNet's own launches -- `ia2p_gemm` (plain and GEGLU), `ia2p_gemm_splitk`, `ia2p_gemm_ex` (row statistics and the folded LayerNorm), the 3x3 and boundary
convolutions, the GroupNorm column sums of `ia2p_gemm_gnstats`, `ia2p_conv3x3_gn` and `ia2p_gn_colstats`, `ia2p_gn_apply_stats`, `ia2p_groupnorm_silu`, `ia2p_layernorm`, the element-wise sampler steps and `ia2p_linear_small` -- one by one against the fp64 references of
tests/unet_ops_ref.py.

The GEMM and convolution inputs lie on a lattice on which every fp32 accumulation is exact in any order (unet_ops_ref's docstring; test_unet_ops_cpu.py asserts the
conditions for every case used here), so the plain epilogues are held to the exact bits of fp64 and the others to the few fp32 operations behind the accumulator.
Every output element is compared. Every launch runs twice into NaN-filled outputs between guard regions and must give the same bits; max(err / bound) is printed per
test (pytest -s; docs/LOG.md §32 records a run)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
_INT = {torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
IN_LAUNCH, REDUCE_LAUNCH = 1 << 40, 0


@pytest.fixture(scope="module")
def L():
    from instructany2pix_amd import _ffi
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = _ffi.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    yield lib
    lib.ia2p_debug_set_gemm_tile(-1)
    lib.ia2p_debug_set_splitk_inkernel(-1)


def _ffi():
    from instructany2pix_amd import _ffi as f
    return f


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _report(tag, worst):
    print(f"[unet-ops] {tag}: max(err / bound) {worst:.4g}")


class Out:
    """an output buffer of n elements filled with NaN, GUARD elements in front of it and behind it"""

    def __init__(self, n, dtype=torch.float16):
        self.n, self.dtype = int(n), dtype
        self.buf = torch.empty(2 * GUARD + self.n, dtype=dtype, device=DEV)
        self.reset()

    def reset(self, init=None):
        self.buf.fill_(float("nan"))
        if init is not None:
            self.out.copy_(init.reshape(-1))
        self.guards = [g.view(_INT[self.dtype]).clone() for g in (self.buf[:GUARD], self.buf[GUARD + self.n:])]

    @property
    def out(self):
        return self.buf[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def check(self, tag):
        now = [g.view(_INT[self.dtype]) for g in (self.buf[:GUARD], self.buf[GUARD + self.n:])]
        assert torch.equal(now[0], self.guards[0]), f"{tag}: wrote in front of its output"
        assert torch.equal(now[1], self.guards[1]), f"{tag}: wrote behind its output"


def _twice(tag, launch, outs, init=None, partly=()):
    """launch twice from freshly filled buffers: the status is OK, same bits, guards intact, every output written (the buffers in `partly` may be written in part: the
    caller checks which part). -> the outputs (on the CPU)"""
    f = _ffi()
    bits = []
    for _ in range(2):
        for o in outs:
            o.reset(init)
        f.check(launch())
        torch.cuda.synchronize()
        bits.append([o.buf.view(_INT[o.dtype]).clone() for o in outs])
    for a, b in zip(*bits):
        assert torch.equal(a, b), f"{tag}: a second launch gives other bits"
    for o in outs:
        o.check(tag)
        assert o in partly or bool(torch.isfinite(o.out.double()).all()), f"{tag}: an output is not finite (or was never written)"
    return [o.out.cpu() for o in outs]


# ---- 1. ia2p_gemm, plain epilogue: the exact bits on all 28 tiles -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", R.GEMM_SHAPES)
def test_gemm_plain_epilogue_is_fp64_to_the_bit(L, M, N, K):
    f = _ffi()
    c = R.gemm_case(M, N, K)
    A, W, b, res = _d(c["A"]), _d(c["W"]), _d(c["bias"]), _d(c["res"])
    o = Out(M * N)
    try:
        for epi in R.GEMM_EPILOGUES:
            ref, _ = R.gemm_ref(c, epi)
            bias = b if "bias" in epi else None
            for tile in R.ALL_TILES:
                L.ia2p_debug_set_gemm_tile(tile)
                tag = f"gemm {M}x{N}x{K} {epi} tile {tile}"
                if "aliased" in epi:          # the residual is read from the output buffer itself
                    got = _twice(tag, lambda: L.ia2p_gemm(f.current_stream(), _p(A), _p(W), _p(bias), o.ptr, o.ptr, M, N, K, 0), [o], init=res)[0]
                else:
                    got = _twice(tag, lambda: L.ia2p_gemm(f.current_stream(), _p(A), _p(W), _p(bias), _p(res if "residual" in epi else None), o.ptr, M, N, K, 0), [o])[0]
                R.accept(tag, got, ref, None, ("m", "n"))
    finally:
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"gemm {M}x{N}x{K}", 0.0)


# ---- 2. ia2p_gemm_splitk: both finish routes, poisoned slabs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,S", R.SPLITK_SHAPES)
def test_gemm_splitk_is_fp64_to_the_bit(L, M, N, K, S):
    f = _ffi()
    c = R.gemm_case(M, N, K)
    A, W, b, res = _d(c["A"]), _d(c["W"]), _d(c["bias"]), _d(c["res"])
    ref, _ = R.gemm_ref(c)
    o = Out(M * N)
    part = torch.empty(S * M * N, dtype=torch.float32, device=DEV)

    def launch():
        part.fill_(float("nan"))          # a slab read before it is written, or never written, poisons the output
        return L.ia2p_gemm_splitk(f.current_stream(), _p(A), _p(W), _p(b), _p(res), o.ptr, M, N, K, S, _p(part))
    try:
        for route, limit in (("in-launch", IN_LAUNCH), ("reduce launch", REDUCE_LAUNCH)):
            L.ia2p_debug_set_splitk_inkernel(limit)
            for tile in R.SPLITK_TILES:
                L.ia2p_debug_set_gemm_tile(tile)
                tag = f"gemm_splitk {M}x{N}x{K}/{S} {route} tile {tile}"
                R.accept(tag, _twice(tag, launch, [o])[0], ref, None, ("m", "n"))
    finally:
        L.ia2p_debug_set_splitk_inkernel(-1)
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"gemm_splitk {M}x{N}x{K}/{S}", 0.0)


# ---- 3. GEGLU ------------------------------------------------------------------------------------------------------------------------------------------------------
def _pack_geglu(L, W, b):
    f = _ffi()
    N, K = W.shape
    Wp, bp = torch.empty_like(W), torch.empty_like(b)
    f.check(L.ia2p_pack_geglu(f.current_stream(), _p(W), _p(Wp), N, K))
    f.check(L.ia2p_pack_geglu(f.current_stream(), _p(b), _p(bp), N, 1))
    torch.cuda.synchronize()
    return Wp, bp


@pytest.mark.parametrize("M,N,K", R.GEGLU_SHAPES)
def test_gemm_geglu_within_the_table_bound(L, M, N, K):
    f = _ffi()
    c = R.geglu_case(M, N, K)
    ref, bound = R.geglu_ref(c)
    A = _d(c["A"])
    Wp, bp = _pack_geglu(L, _d(c["W"]), _d(c["bias"]))
    o = Out(M * N // 2)
    worst = 0.0
    try:
        for tile in R.GEGLU_TILES:
            L.ia2p_debug_set_gemm_tile(tile)
            tag = f"geglu {M}x{N}x{K} tile {tile}"
            got = _twice(tag, lambda: L.ia2p_gemm(f.current_stream(), _p(A), _p(Wp), _p(bp), None, o.ptr, M, N, K, 1), [o])[0]
            worst = max(worst, R.accept(tag, got, ref, bound, ("m", "n")))
    finally:
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"geglu {M}x{N}x{K}", worst)


# ---- 4. row statistics and the folded LayerNorm, ia2p_gemm_ex ---------------------------------------------------------------------------------------------------
def _fold(L, W, gamma, beta, bias):
    f = _ffi()
    N, K = W.shape
    Wf = torch.full_like(W, float("nan"))
    cs, lb = torch.full((N,), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    f.check(L.ia2p_fold_layernorm(f.current_stream(), _p(W), _p(gamma), _p(beta), _p(bias), _p(Wf), _p(cs), _p(lb), N, K))
    torch.cuda.synchronize()
    return Wf, cs, lb


def _produce(L, c, tile, psplit, part):
    """the producer launch -> t (fp16, CPU), the summed slots [M, 2] (fp64, CPU), the device tensors the consumer reads (t, stats, slots)"""
    f = _ffi()
    M, K = c["M"], c["C"]
    X, Wp, Rr = _d(c["X"]), _d(c["Wp"]), _d(c["R"])
    t = Out(M * K)
    stats = torch.zeros((K // 64 + 1) * M * 2, dtype=torch.float32, device=DEV)
    slots = C.c_int(0)

    def launch():
        stats.fill_(float("nan"))
        part.fill_(float("nan"))
        return L.ia2p_gemm_ex(f.current_stream(), _p(X), _p(Wp), None, _p(Rr), t.ptr, M, K, K, 0, None, _p(stats), C.addressof(slots), psplit, _p(part))
    tag = f"ln producer {M}x{K} tile {tile} split {psplit}"
    L.ia2p_debug_set_gemm_tile(tile)
    got = _twice(tag, launch, [t])[0]
    assert slots.value >= 1, tag
    st = stats.view(-1, M, 2)[:slots.value].double().cpu()
    assert bool(torch.isfinite(st).all()), f"{tag}: a statistics slot was never written"
    tf = t.out.float().view(M, K)
    sum_ = stats.view(-1, M, 2)[:slots.value].sum(0)
    assert torch.allclose(sum_[:, 0], tf.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(sum_[:, 1], (tf * tf).sum(1), rtol=1e-4, atol=1e-2)
    return got, st.sum(0), (t, stats, slots.value)


@pytest.mark.parametrize("M,C_,N", R.LNFOLD_SHAPES)
def test_layernorm_fold_statistics_exact_and_output_within_the_fp32_bound(L, M, C_, N):
    f = _ffi()
    c = R.lnfold_case(M, C_, N)
    t_ref, st_ref = R.lnfold_producer(c)
    Wf_ref, cs_ref, (lb_ref, lb_bound) = R.lnfold_weights(c)
    h, E = R.lnfold_ref(c, t_ref)
    bound = R.with_store16(h, E)
    Wf, cs, lb = _fold(L, _d(c["W"]), _d(c["gamma"]), _d(c["beta"]), _d(c["bias"]))
    R.accept("fold Wf", Wf.cpu(), Wf_ref, None, ("n", "k"))
    R.accept("fold colsum", cs.cpu(), cs_ref, None, ("n",))
    worst_lb = R.accept("fold bias", lb.cpu(), lb_ref, lb_bound, ("n",))
    part = torch.empty(4 * M * max(N, C_), dtype=torch.float32, device=DEV)
    o = Out(M * N)
    worst = 0.0
    try:
        for tile in R.LNFOLD_TILES:
            for psplit in (1, 2):
                got_t, st, (t, stats, slots) = _produce(L, c, tile, psplit, part)
                R.accept(f"ln producer t tile {tile} split {psplit}", got_t, t_ref, None, ("m", "k"))
                R.accept(f"ln producer statistics tile {tile} split {psplit}", st, st_ref, None, ("m", "sum | sum of squares"))
            ln = f.LnFoldC(stats.data_ptr(), slots, cs.data_ptr(), lb.data_ptr(), c["eps"])
            for csplit in (1, 2):
                tag = f"ln consumer {M}x{C_}->{N} tile {tile} split {csplit}"

                def launch():
                    part.fill_(float("nan"))
                    return L.ia2p_gemm_ex(f.current_stream(), t.ptr, _p(Wf), None, None, o.ptr, M, N, C_, 0, C.addressof(ln), None, None, csplit, _p(part))
                worst = max(worst, R.accept(tag, _twice(tag, launch, [o])[0], h, bound, ("m", "n")))
    finally:
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"ln fold {M}x{C_}->{N} (fold bias {worst_lb:.3g})", worst)


@pytest.mark.parametrize("M,C_,N", [(77, 128, 512), (300, 256, 768)])
def test_layernorm_fold_into_geglu_within_the_bound(L, M, C_, N):
    f = _ffi()
    c = R.lnfold_case(M, C_, N, geglu=True)
    t_ref, _ = R.lnfold_producer(c)
    h, E = R.lnfold_ref(c, t_ref)
    E16 = R.with_store16(h, E)
    H = N // 2
    ref, bound = R.geglu_apply(h[:, :H], h[:, H:], E16[:, :H], E16[:, H:])
    Wp, bp = _pack_geglu(L, _d(c["W"]), _d(c["bias"]))
    Wf, cs, lb = _fold(L, Wp, _d(c["gamma"]), _d(c["beta"]), bp)
    part = torch.empty(4 * M * max(N, C_), dtype=torch.float32, device=DEV)
    o = Out(M * H)
    worst = 0.0
    try:
        _, _, (t, stats, slots) = _produce(L, c, -1, 1, part)
        ln = f.LnFoldC(stats.data_ptr(), slots, cs.data_ptr(), lb.data_ptr(), c["eps"])
        for tile in R.LNFOLD_GEGLU_TILES:
            L.ia2p_debug_set_gemm_tile(tile)
            tag = f"ln fold geglu {M}x{C_}->{N} tile {tile}"
            got = _twice(tag, lambda: L.ia2p_gemm_ex(f.current_stream(), t.ptr, _p(Wf), None, None, o.ptr, M, N, C_, 1, C.addressof(ln), None, None, 1, None), [o])[0]
            worst = max(worst, R.accept(tag, got, ref, bound, ("m", "n")))
    finally:
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"ln fold geglu {M}x{C_}->{N}", worst)


# ---- 5. convolutions ---------------------------------------------------------------------------------------------------------------------------------------------
def _pack3(L, w):
    f = _ffi()
    Co, Cin = w.shape[:2]
    wp = torch.full((Co, 9 * Cin), float("nan"), dtype=torch.half, device=DEV)
    f.check(L.ia2p_pack_conv3x3(f.current_stream(), _p(w), _p(wp), Co, Cin))
    torch.cuda.synchronize()
    return wp


@pytest.mark.parametrize("B,H,W,Cin,Co,stride,up", R.CONV_SHAPES)
def test_conv3x3_is_fp64_to_the_bit(L, B, H, W, Cin, Co, stride, up):
    f = _ffi()
    shape = (B, H, W, Cin, Co, stride, up)
    c = R.conv_case(*shape)
    ref, _ = R.conv_ref(c)
    x, b, tv, res = _d(c["x"]), _d(c["bias"]), _d(c["tv"]), _d(c["res"])
    wp = _pack3(L, _d(c["w"]))
    o = Out(ref.numel())
    tiles = R.ALL_TILES if shape in R.CONV_ALL_TILES else (-1, 0, 4, 8, 12, 18, 20, 22)
    if shape in R.CONV_HALO:
        tiles = tuple(tiles) + tuple(t for t in (24, 25, 26) if t not in tiles)
    M = B * c["Ho"] * c["Wo"]
    part = torch.empty(3 * M * Co, dtype=torch.float32, device=DEV)
    try:
        for tile in tiles:
            L.ia2p_debug_set_gemm_tile(tile)
            tag = f"conv3x3 {shape} tile {tile}"
            got = _twice(tag, lambda: L.ia2p_conv3x3(f.current_stream(), _p(x), _p(wp), _p(b), _p(tv), _p(res), o.ptr, B, H, W, Cin, Co, stride, up), [o])[0]
            R.accept(tag, got, ref, None, R.CONV_AXES)
        if stride == 1 and not up:
            for route, limit in (("in-launch", IN_LAUNCH), ("reduce launch", REDUCE_LAUNCH)):
                L.ia2p_debug_set_splitk_inkernel(limit)
                for tile in (-1, 0, 12) + ((24, 25, 26) if shape in R.CONV_HALO else ()):
                    L.ia2p_debug_set_gemm_tile(tile)
                    for sk in (1, 2, 3):
                        tag = f"conv3x3_splitk {shape} {route} tile {tile} split {sk}"

                        def launch():
                            part.fill_(float("nan"))
                            return L.ia2p_conv3x3_splitk(f.current_stream(), _p(x), _p(wp), _p(b), _p(tv), _p(res), o.ptr, B, H, W, Cin, Co, sk, _p(part))
                        R.accept(tag, _twice(tag, launch, [o])[0], ref, None, R.CONV_AXES)
    finally:
        L.ia2p_debug_set_splitk_inkernel(-1)
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"conv3x3 {shape}", 0.0)


@pytest.mark.parametrize("B,H,W,Cin,Cin2,Co", R.CONV_CAT_SHAPES)
def test_conv3x3_cat_is_fp64_to_the_bit(L, B, H, W, Cin, Cin2, Co):
    f = _ffi()
    c = R.conv_case(B, H, W, Cin, Co, Cin2=Cin2)
    ref, _ = R.conv_ref(c)
    h, x2, b = _d(c["x"]), _d(c["x2"]), _d(c["bias"])
    wcat = torch.cat([_pack3(L, _d(c["w"])), _d(c["wsc"])], dim=1).contiguous()
    o = Out(ref.numel())
    try:
        for tile in (-1, 0, 4, 6, 8, 12, 16, 20, 24, 25, 26):
            L.ia2p_debug_set_gemm_tile(tile)
            tag = f"conv3x3_cat {(B, H, W, Cin, Cin2, Co)} tile {tile}"
            got = _twice(tag, lambda: L.ia2p_conv3x3_cat(f.current_stream(), _p(h), _p(x2), _p(wcat), _p(b), o.ptr, B, H, W, Cin, Cin2, Co), [o])[0]
            R.accept(tag, got, ref, None, R.CONV_AXES)
    finally:
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"conv3x3_cat {(B, H, W, Cin, Cin2, Co)}", 0.0)


@pytest.mark.parametrize("B,Cin,H,W,Co", R.CONV_IN_SHAPES)
def test_conv_in_is_fp64_to_the_bit(L, B, Cin, H, W, Co):
    f = _ffi()
    c = R.boundary_case("in", B, Cin, H, W, Co)
    ref, _ = R.boundary_ref(c)
    x = _d(c["x"].permute(0, 3, 1, 2))          # NCHW
    w, b = _d(c["w"]), _d(c["bias"])
    ws = torch.full((Co * 64,), float("nan"), dtype=torch.half, device=DEV)
    o = Out(ref.numel())
    tag = f"conv_in {(B, Cin, H, W, Co)}"
    got = _twice(tag, lambda: L.ia2p_conv_in(f.current_stream(), _p(x), _p(w), _p(b), o.ptr, _p(ws), B, Cin, H, W, Co), [o])[0]
    R.accept(tag, got, ref, None, R.CONV_AXES)
    _report(tag, 0.0)


@pytest.mark.parametrize("B,C_,H,W,Co", R.CONV_OUT_SHAPES)
def test_conv_out_is_fp64_to_the_bit(L, B, C_, H, W, Co):
    f = _ffi()
    c = R.boundary_case("out", B, C_, H, W, Co)
    ref, _ = R.boundary_ref(c)
    x, w, b = _d(c["x"]), _d(c["w"]), _d(c["bias"])
    wp = torch.full((Co * 9 * C_,), float("nan"), dtype=torch.half, device=DEV)
    f.check(L.ia2p_pack_conv_out(f.current_stream(), _p(w), _p(wp), Co, C_))
    o = Out(ref.numel())
    tag = f"conv_out {(B, C_, H, W, Co)}"
    got = _twice(tag, lambda: L.ia2p_conv_out(f.current_stream(), _p(x), _p(wp), _p(b), o.ptr, B, C_, H, W, Co), [o])[0]
    R.accept(tag, got.reshape(B, Co, H, W).permute(0, 2, 3, 1), ref, None, R.CONV_AXES)          # NCHW out
    _report(tag, 0.0)


def _colstats(L, x2d, rows, tag):
    f = _ffi()
    M, Cc = x2d.shape
    o = Out(M // rows * Cc * 2, torch.float64)
    return _twice(tag, lambda: L.ia2p_gn_colstats(f.current_stream(), _p(x2d), M, Cc, rows, o.ptr), [o])[0].reshape(M // rows, Cc, 2), o


@pytest.mark.parametrize("B,HW,C_,C0,rows0,rows1", R.GN_STATS_SHAPES)
def test_gn_colstats_exact_and_apply_stats_within_the_groupnorm_bound(L, B, HW, C_, C0, rows0, rows1):
    """ia2p_gn_colstats on the lattice: the fp64 column sums to the bit; ia2p_gn_apply_stats from those sums (one source, or two that are never concatenated):
    the GroupNorm bound of the lattice case. (ia2p_conv3x3_gn is held through them: test_gn_fused_gpu.py pins it bit for bit to this pass followed by the plain
    halo-staged convolution, which test_conv3x3_is_fp64_to_the_bit pins on the lattice.)"""
    f = _ffi()
    c = R.gn_case(B, HW, C_)
    x = c["x"].reshape(B * HW, C_)
    x0, x1 = _d(x[:, :C0]), (_d(x[:, C0:]) if C0 < C_ else None)
    ga, be = _d(c["gamma"]), _d(c["beta"])
    st0, keep0 = _colstats(L, x0, rows0, "gn_colstats source 0")
    R.accept("gn_colstats source 0", st0, R.colstats_ref(x[:, :C0], rows0), None, ("slot", "c", "sum | sum of squares"))
    keep1 = None
    if x1 is not None:
        st1, keep1 = _colstats(L, x1, rows1, "gn_colstats source 1")
        R.accept("gn_colstats source 1", st1, R.colstats_ref(x[:, C0:], rows1), None, ("slot", "c", "sum | sum of squares"))
    o = Out(B * HW * C_)
    worst = 0.0
    for silu in (1, 0):
        ref, bound, _ = R.gn_ref(c, silu, 1e-5)
        tag = f"gn_apply_stats {(B, HW, C_, C0)} silu {silu}"
        got = _twice(tag, lambda: L.ia2p_gn_apply_stats(f.current_stream(), _p(x0), C0, keep0.ptr, rows0, _p(x1), C_ - C0, keep1.ptr if keep1 else None, rows1,
                                                        _p(ga), _p(be), o.ptr, B, HW, R.GN_GROUPS, 1e-5, silu), [o])[0]
        worst = max(worst, R.accept(tag, got.reshape(B, HW, C_), ref, bound, ("b", "pixel", "c")))
    _report(f"gn_colstats + gn_apply_stats {(B, HW, C_, C0)}", worst)


def _used_statistics(tag, st, used):
    """the first `used` doubles of a statistics buffer are written and nothing behind them is"""
    assert bool(torch.isfinite(st[:used]).all()), f"{tag}: a column sum was never written"
    assert bool(torch.isnan(st[used:]).all()), f"{tag}: wrote behind the {used} column sums it reported"
    return st[:used]


@pytest.mark.parametrize("M,N,K,HW", R.GEMM_GNSTATS_SHAPES)
def test_gemm_gnstats_output_and_column_sums_exact(L, M, N, K, HW):
    """ia2p_gemm_gnstats on the lattice: the output to the bit, and the column sums its epilogue leaves are the fp64 sums of that output, on linear tiles of 64 .. 256
    rows; with two k-tiles also under a K split finished inside the launch (finished by the reduce launch it reports no statistics: rows = 0)"""
    f = _ffi()
    c = R.gemm_gnstats_case(M, N, K, HW)
    ref, _ = R.gemm_ref(c, "bias")
    A, W, b = _d(c["A"]), _d(c["W"]), _d(c["bias"])
    o, st = Out(M * N), Out(M // 16 * N * 2, torch.float64)
    part = torch.empty(2 * M * N, dtype=torch.float32, device=DEV)
    produced = {0: 0, 2: 0}
    try:
        for route, limit in (("in-launch", IN_LAUNCH), ("reduce launch", REDUCE_LAUNCH)):
            L.ia2p_debug_set_splitk_inkernel(limit)
            for tile in (-1, 0, 2, 4, 8, 12, 16, 18, 19, 20, 22):
                L.ia2p_debug_set_gemm_tile(tile)
                for sk in (0, 2):
                    if sk > K // 64 or (limit == REDUCE_LAUNCH and sk == 0):
                        continue
                    rows = C.c_int(0)
                    tag = f"gemm_gnstats {M}x{N}x{K} {route} tile {tile} split {sk}"

                    def launch():
                        part.fill_(float("nan"))
                        return L.ia2p_gemm_gnstats(f.current_stream(), _p(A), _p(W), _p(b), None, o.ptr, M, N, K, sk, _p(part), HW, st.ptr, C.byref(rows))
                    got, gst = _twice(tag, launch, [o, st], partly=(st,))
                    R.accept(tag, got, ref, None, ("m", "n"))
                    if limit == REDUCE_LAUNCH:
                        assert rows.value == 0, tag
                    if not rows.value:          # (a tile or a route that leaves no statistics: the executor runs ia2p_gn_colstats)
                        _used_statistics(tag, gst, 0)
                        continue
                    gst = _used_statistics(tag, gst, M // rows.value * N * 2)
                    R.accept(tag + " column sums", gst.reshape(M // rows.value, N, 2), R.colstats_ref(ref, rows.value), None, ("slot", "n", "sum | sum of squares"))
                    produced[sk] += 1
    finally:
        L.ia2p_debug_set_splitk_inkernel(-1)
        L.ia2p_debug_set_gemm_tile(-1)
    assert produced[0] >= 6 and (K < 128 or produced[2] >= 6), produced
    _report(f"gemm_gnstats {M}x{N}x{K}", 0.0)


@pytest.mark.parametrize("B,H,W,Cin,Co", R.CONV_GNSTATS_SHAPES)
def test_conv3x3_gn_producer_form_output_and_column_sums_exact(L, B, H, W, Cin, Co):
    """ia2p_conv3x3_gn without input statistics (a plain convolution that leaves the GroupNorm column sums of its output) on the lattice: the output to the bit of fp64,
    and the column sums are the fp64 sums of that output -- slot by slot on the linear tiles, per image on the halo-staged tiles 24 .. 26, whose slots are 16 x 16
    patches -- unsplit and with a K split finished inside the launch. (The consumer form, with input statistics, multiplies normalised activations, which are on no
    lattice: test_gn_fused_gpu.py pins it bit for bit to ia2p_gn_apply_stats followed by this form.)"""
    f = _ffi()
    c = R.conv_gnstats_case(B, H, W, Cin, Co)
    ref, _ = R.conv_ref(c)
    HW, M = H * W, B * H * W
    ref2d = ref.reshape(M, Co)
    x, b = _d(c["x"]), _d(c["bias"])
    wp = _pack3(L, _d(c["w"]))
    o, st = Out(M * Co), Out(M // 16 * Co * 2, torch.float64)
    part = torch.empty(3 * M * Co, dtype=torch.float32, device=DEV)
    d = f.ConvGnC()
    d.x0, d.C0, d.Wp, d.bias, d.y = x.data_ptr(), Cin, wp.data_ptr(), b.data_ptr(), o.ptr.value
    d.B, d.H, d.W, d.Co, d.groups, d.eps = B, H, W, Co, 32, 1e-5
    d.partial, d.gn_out = part.data_ptr(), st.ptr.value
    produced = {"halo": 0, "linear": 0, "split": 0}
    try:
        L.ia2p_debug_set_splitk_inkernel(IN_LAUNCH)
        for tile in (24, 25, 26, 18, 12, 0, 4, 8, 16, 19, 22):
            L.ia2p_debug_set_gemm_tile(tile)
            for sk in (0, 2, 3):
                d.splitk = sk
                rows = C.c_int(0)
                tag = f"conv3x3_gn producer {(B, H, W, Cin, Co)} tile {tile} split {sk}"

                def launch():
                    part.fill_(float("nan"))
                    return L.ia2p_conv3x3_gn(f.current_stream(), C.byref(d), C.byref(rows))
                got, gst = _twice(tag, launch, [o, st], partly=(st,))
                R.accept(tag, got.reshape(B, H, W, Co), ref, None, R.CONV_AXES)
                if not rows.value:          # (a tile that does not divide the image leaves no statistics)
                    _used_statistics(tag, gst, 0)
                    continue
                gst = _used_statistics(tag, gst, M // rows.value * Co * 2).reshape(M // rows.value, Co, 2)
                want = R.colstats_ref(ref2d, rows.value)
                per_image = lambda t: t.reshape(B, HW // rows.value, Co, 2).sum(1)      # noqa: E731
                R.accept(tag + " column sums per image", per_image(gst), per_image(want), None, ("b", "co", "sum | sum of squares"))
                if tile not in (24, 25, 26):
                    R.accept(tag + " column sums", gst, want, None, ("slot", "co", "sum | sum of squares"))
                produced["halo" if tile in (24, 25, 26) else "linear"] += 1
                produced["split"] += sk > 1
    finally:
        L.ia2p_debug_set_splitk_inkernel(-1)
        L.ia2p_debug_set_gemm_tile(-1)
    assert produced["halo"] >= 3 and produced["linear"] >= 3 and produced["split"] >= 3, produced
    _report(f"conv3x3_gn producer {(B, H, W, Cin, Co)}", 0.0)


# ---- 6. GroupNorm (+ SiLU) and LayerNorm -----------------------------------------------------------------------------------------------------------------------
def _groupnorm(L, c, silu, eps, tag):
    """-> (y on the CPU, the route taken: the two-pass kernels write their chunk partials, the single pass leaves the buffer alone)"""
    f = _ffi()
    B, HW, C_ = c["B"], c["HW"], c["C"]
    x, ga, be = _d(c["x"]), _d(c["gamma"]), _d(c["beta"])
    part = torch.empty(B * 64 * R.GN_GROUPS * 2, dtype=torch.float32, device=DEV)
    o = Out(B * HW * C_)

    def launch():
        part.fill_(float("nan"))
        return L.ia2p_groupnorm_silu(f.current_stream(), _p(x), o.ptr, _p(ga), _p(be), B, HW, C_, R.GN_GROUPS, eps, silu, _p(part))
    got = _twice(tag, launch, [o])[0].reshape(B, HW, C_)
    return got, "twopass" if bool(torch.isfinite(part).any()) else "fused"


@pytest.mark.parametrize("silu,eps", R.GN_VARIANTS)
@pytest.mark.parametrize("B,HW,C_", R.GN_SHAPES)
def test_groupnorm_silu_lattice_within_the_fp32_bound(L, B, HW, C_, silu, eps):
    c = R.gn_case(B, HW, C_)
    ref, bound, _ = R.gn_ref(c, silu, eps)
    tag = f"groupnorm {(B, HW, C_)} silu {silu} eps {eps}"
    got, route = _groupnorm(L, c, silu, eps, tag)
    assert route == R.gn_route(B, HW, C_)[0], (tag, route, R.gn_route(B, HW, C_))          # the implementation the case was chosen for is the one that ran
    _report(tag + f" {R.gn_route(B, HW, C_)}", R.accept(tag, got, ref, bound, ("b", "pixel", "c")))


@pytest.mark.parametrize("B,HW,C_", R.GN_REAL_SHAPES)
def test_groupnorm_silu_real_values_far_from_zero(L, B, HW, C_):
    c = R.gn_case(B, HW, C_, real=True)
    worst = 0.0
    for silu in (1, 0):
        ref, bound, _ = R.gn_ref(c, silu, 1e-5)
        tag = f"groupnorm real {(B, HW, C_)} silu {silu}"
        got, route = _groupnorm(L, c, silu, 1e-5, tag)
        assert route == R.gn_route(B, HW, C_)[0], (tag, route)
        worst = max(worst, R.accept(tag, got, ref, bound, ("b", "pixel", "c")))
    _report(f"groupnorm real {(B, HW, C_)}", worst)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("M,C_", R.LN_SHAPES)
def test_layernorm_lattice_within_the_fp32_bound(L, M, C_, eps):
    f = _ffi()
    c = R.ln_case(M, C_)
    ref, bound = R.ln_ref(c, eps)
    x, ga, be = _d(c["x"]), _d(c["gamma"]), _d(c["beta"])
    o = Out(M * C_)
    tag = f"layernorm {(M, C_)} eps {eps}"
    got = _twice(tag, lambda: L.ia2p_layernorm(f.current_stream(), _p(x), o.ptr, _p(ga), _p(be), M, C_, eps), [o])[0]
    _report(tag, R.accept(tag, got, ref, bound, ("m", "c")))


# ---- 7. element-wise steps and the skinny linear ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C_,HW", R.EW_SIZES)
def test_ddim_step_and_its_per_row_form(L, B, C_, HW):
    f = _ffi()
    c = R.ew_case(B, C_, HW)
    n, per = c["n"], c["per"]
    x, eu, ec = _d(c["x"]), _d(c["eu"]), _d(c["ec"])
    o, o2 = Out(n), Out(n)
    worst = 0.0
    shared = c["ddim_coef"][:1].expand(B, 3).contiguous()
    g, cx, ce = (float(v) for v in shared[0])
    for guided in (True, False):
        e = ec if guided else None
        ref, bound = R.ddim_ref(c, shared, guided)
        tag = f"ddim_step n {n} guided {guided}"
        got, got2 = _twice(tag, lambda: L.ia2p_ddim_step(f.current_stream(), _p(x), _p(eu), _p(e), g, cx, ce, o.ptr, o2.ptr, n), [o, o2])
        assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), f"{tag}: out2 is not out"
        worst = max(worst, R.accept(tag, got, ref, bound))
        coef = _d(shared)
        same = _twice(tag + " coef", lambda: L.ia2p_ddim_step_v(f.current_stream(), _p(x), _p(eu), _p(e), _p(coef), o.ptr, o2.ptr, B, per), [o, o2])[0]
        assert torch.equal(same.view(torch.int16), got.view(torch.int16)), f"{tag}: the coef form with shared scalars gives other bits"
        ref, bound = R.ddim_ref(c, c["ddim_coef"], guided)
        coef = _d(c["ddim_coef"])
        tag = f"ddim_step_v n {n} guided {guided}"
        got, got2 = _twice(tag, lambda: L.ia2p_ddim_step_v(f.current_stream(), _p(x), _p(eu), _p(e), _p(coef), o.ptr, o2.ptr, B, per), [o, o2])
        assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), f"{tag}: out2 is not out"
        worst = max(worst, R.accept(tag, got, ref, bound))
    _report(f"ddim_step(_v) n {n}", worst)


@pytest.mark.parametrize("B,C_,HW", R.EW_SIZES)
def test_mask_blend_and_its_per_row_form(L, B, C_, HW):
    f = _ffi()
    c = R.ew_case(B, C_, HW)
    n = c["n"]
    x, init, noise, mask = _d(c["x"]), _d(c["init"]), _d(c["noise"]), _d(c["mask"])
    o, o2 = Out(n), Out(n)
    shared = c["blend_coef"][:1].expand(B, 2).contiguous()
    c0, c1 = (float(v) for v in shared[0])
    ref, bound = R.blend_ref(c, shared)
    tag = f"mask_blend n {n}"
    got, got2 = _twice(tag, lambda: L.ia2p_mask_blend(f.current_stream(), _p(x), _p(init), _p(noise), _p(mask), c0, c1, o.ptr, o2.ptr, B, C_, HW), [o, o2])
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), f"{tag}: out2 is not out"
    worst = R.accept(tag, got, ref, bound)
    coef = _d(shared)
    same = _twice(tag + " coef", lambda: L.ia2p_mask_blend_v(f.current_stream(), _p(x), _p(init), _p(noise), _p(mask), _p(coef), o.ptr, o2.ptr, B, C_, HW), [o, o2])[0]
    assert torch.equal(same.view(torch.int16), got.view(torch.int16)), f"{tag}: the coef form with shared scalars gives other bits"
    ref, bound = R.blend_ref(c, c["blend_coef"])
    coef = _d(c["blend_coef"])
    tag = f"mask_blend_v n {n}"
    got, got2 = _twice(tag, lambda: L.ia2p_mask_blend_v(f.current_stream(), _p(x), _p(init), _p(noise), _p(mask), _p(coef), o.ptr, o2.ptr, B, C_, HW), [o, o2])
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), f"{tag}: out2 is not out"
    worst = max(worst, R.accept(tag, got, ref, bound))
    _report(f"mask_blend(_v) n {n}", worst)


@pytest.mark.parametrize("B,C_,HW", R.EW_SIZES)
def test_prior_step(L, B, C_, HW):
    f = _ffi()
    c = R.ew_case(B, C_, HW)
    n = c["n"]
    s, oc, ou, nz = _d(c["s"]), _d(c["ec"]), _d(c["eu"]), _d(c["noise32"])
    p = R.PRIOR_SCALARS
    o = Out(n, torch.float32)
    worst = 0.0
    for guided, noisy in ((True, True), (False, True), (True, False)):
        ref, bound = R.prior_ref(c, guided, noisy)
        tag = f"prior_step n {n} guided {guided} noise {noisy}"
        got = _twice(tag, lambda: L.ia2p_prior_step(f.current_stream(), _p(s), _p(oc if guided else None), _p(ou), _p(nz if noisy else None), p["g"], p["sqrt_a"], p["sqrt_b"],
                                                    p["k0"], p["k1"], p["sigma"], o.ptr, n), [o])[0]
        worst = max(worst, R.accept(tag, got, ref, bound))
    _report(f"prior_step n {n}", worst)


@pytest.mark.parametrize("M,N,K", R.LINEAR_SHAPES)
def test_linear_small_is_fp64_to_the_bit(L, M, N, K):
    f = _ffi()
    c = R.linear_case(M, N, K)
    ref, _, _ = R.linear_ref(c)
    X, W, b = _d(c["A"]), _d(c["W"]), _d(c["bias"])
    o = Out(M * N)
    tag = f"linear_small {(M, N, K)}"
    got = _twice(tag, lambda: L.ia2p_linear_small(f.current_stream(), _p(X), _p(W), _p(b), o.ptr, M, N, K, 0, 0), [o])[0]
    R.accept(tag, got, ref, None, ("m", "n"))
    _report(tag, 0.0)


@pytest.mark.parametrize("M,N,K", R.LINEAR_REAL_SHAPES)
def test_linear_small_with_both_silus_within_the_bound(L, M, N, K):
    f = _ffi()
    c = R.linear_case(M, N, K, real=True)
    ref, bound, _ = R.linear_ref(c, 1, 1)
    X, W, b = _d(c["A"]), _d(c["W"]), _d(c["bias"])
    o = Out(M * N)
    tag = f"linear_small silu {(M, N, K)}"
    got = _twice(tag, lambda: L.ia2p_linear_small(f.current_stream(), _p(X), _p(W), _p(b), o.ptr, M, N, K, 1, 1), [o])[0]
    _report(tag, R.accept(tag, got, ref, bound, ("m", "n")))
