"""The ControlNet path's launches one by one against the fp64 references of tests/controlnet_ops_ref.py: every output element compared, every launch made twice into
NaN-filled outputs between guard regions (`_twice`), max(err / bound) printed per test."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controlnet_ops_ref as CO  # noqa: E402
import unet_ops_ref as R  # noqa: E402
from test_unet_ops_gpu import DEV, Out, _d, _ffi, _p, _twice  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from instructany2pix_amd import _ffi as f
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = f.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    yield lib
    lib.ia2p_debug_set_gemm_tile(-1)


def _report(tag, worst):
    print(f"[controlnet-ops] {tag}: max(err / bound) {worst:.4g}")


def _pack(L, w):
    f = _ffi()
    Co, Cin = w.shape[:2]
    wp = torch.full((Co, 9 * Cin), float("nan"), dtype=torch.half, device=DEV)
    f.check(L.ia2p_pack_conv_out(f.current_stream(), _p(w), _p(wp), Co, Cin))
    torch.cuda.synchronize()
    return wp


@pytest.mark.parametrize("B,H,W,Cin,Co,stride", CO.NARROW_SHAPES)
def test_conv3x3_narrow(L, B, H, W, Cin, Co, stride):
    """without SiLU the exact bits; with SiLU within the SiLU bound, the exponential model's share below a tenth"""
    f = _ffi()
    c = CO.narrow_case(B, H, W, Cin, Co, stride)
    x, w, b = _d(c["x"]), _d(c["w"]), _d(c["bias"])
    wp = _pack(L, w)
    worst = 0.0
    for silu in (0, 1):
        ref, bound, share = CO.narrow_ref(c, silu)
        assert share < 0.1
        o = Out(ref.numel())
        tag = f"conv3x3_narrow {(B, H, W, Cin, Co, stride)} silu {silu}"
        got = _twice(tag, lambda: L.ia2p_conv3x3_narrow(f.current_stream(), _p(x), _p(wp), _p(b), o.ptr, B, H, W, Cin, Co, stride, silu), [o])[0]
        worst = max(worst, R.accept(tag, got, ref, bound, R.CONV_AXES))
    _report(f"conv3x3_narrow {(B, H, W, Cin, Co, stride)}", worst)


@pytest.mark.parametrize("B,Cin,H,W,Co", CO.CONV_IN_ACT_SHAPES)
def test_conv_in_act_serves_the_3_to_16_convolution(L, B, Cin, H, W, Co):
    f = _ffi()
    c = CO.conv_in_act_case(B, Cin, H, W, Co)
    x = _d(c["x"].permute(0, 3, 1, 2))          # NCHW, as the condition image arrives
    w, b = _d(c["w"]), _d(c["bias"])
    ws = torch.full((Co * 64,), float("nan"), dtype=torch.half, device=DEV)
    r = R.boundary_ref(c)[0]
    worst = 0.0
    for silu in (0, 1):
        if silu:
            ref, Bf, X = R.silu_bound(r, torch.zeros_like(r))
            bound = R.with_store16(ref, Bf)
            assert float((X / bound).max()) < 0.1
        else:
            ref, bound = r, None
        o = Out(ref.numel())
        tag = f"conv_in_act {(B, Cin, H, W, Co)} silu {silu}"
        got = _twice(tag, lambda: L.ia2p_conv_in_act(f.current_stream(), _p(x), _p(w), _p(b), o.ptr, _p(ws), B, Cin, H, W, Co, silu), [o])[0]
        worst = max(worst, R.accept(tag, got, ref, bound, R.CONV_AXES))
    _report(f"conv_in_act {(B, Cin, H, W, Co)}", worst)


@pytest.mark.parametrize("B,HW,Cc", CO.ROWSCALE_SHAPES)
def test_gemm_rowscale_is_fp64_to_the_bit(L, B, HW, Cc):
    """per-row scales (0, 0.75, 1.5) on every tile the GEMM family has; the scale-0 image is all zeros"""
    f = _ffi()
    c = CO.rowscale_case(B, HW, Cc)
    A, W, b, s = _d(c["A"]), _d(c["W"]), _d(c["bias"]), c["scales"].to(DEV)
    ref, _ = CO.rowscale_ref(c)
    M = B * HW
    o = Out(M * Cc)
    try:
        for tile in R.ALL_TILES:
            L.ia2p_debug_set_gemm_tile(tile)
            tag = f"gemm_rowscale {(B, HW, Cc)} tile {tile}"
            got = _twice(tag, lambda: L.ia2p_gemm_rowscale(f.current_stream(), _p(A), _p(W), _p(b), _p(s), o.ptr, M, Cc, Cc, HW), [o])[0]
            R.accept(tag, got, ref, None, ("m", "n"))
            assert float(got.reshape(B, HW, Cc)[0].abs().max()) == 0.0, f"{tag}: the scale-0 image is not all zeros"
    finally:
        L.ia2p_debug_set_gemm_tile(-1)
    _report(f"gemm_rowscale {(B, HW, Cc)}", 0.0)


@pytest.mark.parametrize("B,HW,Cc", CO.INJECT_SHAPES)
def test_residual_add_gnstats(L, B, HW, Cc):
    """fp16(x + r) to the bit, out of place and in place; the column sums are colstats_ref of the result and, bit for bit, ia2p_gn_colstats of it; nothing is written
    behind the statistics; without statistics the same sum"""
    f = _ffi()
    c = CO.inject_case(B, HW, Cc)
    M = c["M"]
    x, r = _d(c["x"]), _d(c["r"])
    ref = CO.inject_ref(c)
    for rows in CO.INJECT_ROWS[(B, HW, Cc)]:
        st_ref = R.colstats_ref(ref, rows)
        for inplace in (False, True):
            o, st = Out(M * Cc), Out((M // rows) * Cc * 2, torch.float64)
            tag = f"residual_add_gnstats {(B, HW, Cc)} rows {rows} {'in place' if inplace else 'out of place'}"
            launch = lambda: L.ia2p_residual_add_gnstats(f.current_stream(), o.ptr if inplace else _p(x), _p(r), o.ptr, M, Cc, rows, st.ptr)      # noqa: E731
            got, gst = _twice(tag, launch, [o, st], init=None) if not inplace else _twice_inplace(tag, launch, o, st, c["x"])
            R.accept(tag, got, ref, None, ("m", "c"))
            R.accept(tag + " column sums", gst.reshape(M // rows, Cc, 2), st_ref, None, ("slot", "c", "sum | sum of squares"))
            y = _d(got.half().reshape(M, Cc))
            cs = Out((M // rows) * Cc * 2, torch.float64)
            canon = _twice(tag + " gn_colstats", lambda: L.ia2p_gn_colstats(f.current_stream(), _p(y), M, Cc, rows, cs.ptr), [cs])[0]
            assert torch.equal(gst.view(torch.int64), canon.view(torch.int64)), f"{tag}: not the bits of ia2p_gn_colstats"
    o = Out(M * Cc)
    got = _twice(f"residual_add {(B, HW, Cc)}", lambda: L.ia2p_residual_add_gnstats(f.current_stream(), _p(x), _p(r), o.ptr, M, Cc, 0, None), [o])[0]
    R.accept(f"residual_add {(B, HW, Cc)}", got, ref, None, ("m", "c"))
    _report(f"residual_add_gnstats {(B, HW, Cc)}", 0.0)


def _twice_inplace(tag, launch, o, st, x):
    """_twice for y == x: the output buffer holds x before each launch"""
    f = _ffi()
    bits = []
    for _ in range(2):
        o.reset(x)
        st.reset()
        f.check(launch())
        torch.cuda.synchronize()
        bits.append([b.buf.view(torch.int16 if b is o else torch.int64).clone() for b in (o, st)])
    for a, b in zip(*bits):
        assert torch.equal(a, b), f"{tag}: a second launch gives other bits"
    for b in (o, st):
        b.check(tag)
        assert bool(torch.isfinite(b.out.double()).all()), f"{tag}: an output is not finite (or was never written)"
    return o.out.cpu(), st.out.cpu()
