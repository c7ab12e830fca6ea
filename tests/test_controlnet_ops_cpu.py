"""The lattice conditions of tests/controlnet_ops_ref.py for every case the GPU tests run, the references against plain torch, and what the four operator entry points
refuse without a device."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controlnet_ops_ref as CO  # noqa: E402
import unet_ops_ref as R  # noqa: E402


@pytest.mark.parametrize("shape", CO.NARROW_SHAPES)
def test_narrow_cases_are_exact_and_the_reference_is_torch_conv(shape):
    c = CO.narrow_case(*shape)
    assert R.exactness(c) < R.LIMIT
    B, H, W, Cin, Co, stride = shape
    assert (c["Ho"], c["Wo"]) == ((H - 1) // stride + 1, (W - 1) // stride + 1)
    want = torch.nn.functional.conv2d(c["x"].double().permute(0, 3, 1, 2), c["w"].double(), c["bias"].double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    ref, bound, _ = CO.narrow_ref(c, 0)
    assert bound is None and torch.equal(ref, R.round16(want))
    assert bool((ref != want).any()) and bool((ref == want).any())          # some outputs need the fp16 rounding, some do not
    out, bound, share = CO.narrow_ref(c, 1)
    assert share < 0.1 and bool((bound > 0).all())
    assert torch.allclose(out, torch.nn.functional.silu(ref))


@pytest.mark.parametrize("shape", CO.CONV_IN_ACT_SHAPES)
def test_conv_in_act_case_is_exact(shape):
    c = CO.conv_in_act_case(*shape)
    assert R.exactness(c) < R.LIMIT
    r = R.boundary_ref(c)[0]
    _, bound, X = R.silu_bound(r, torch.zeros_like(r))
    assert float((X / R.with_store16(r, bound)).max()) < 0.1


@pytest.mark.parametrize("shape", CO.ROWSCALE_SHAPES)
def test_rowscale_cases_are_exact(shape):
    for scales in (CO.ROWSCALE_SCALES, CO.SCALES):
        c = CO.rowscale_case(*shape, scales=scales)
        assert R.exactness(c) < R.LIMIT
        ref, bound = CO.rowscale_ref(c)
        assert bound is None
        B, HW, Cc = shape
        rows = ref.reshape(B, HW, Cc)
        assert float(rows[0].abs().max()) == 0.0                              # the scale-0 image
        plain = R.gemm_ref(c, "bias")[0].reshape(B, HW, Cc)
        sb = R.f64(c["scales"]).reshape(B, 1, 1)
        assert not ({0.75, 1.5} & set(c["scales"].tolist())) or bool((rows != plain * sb).any())                               # the second rounding acts (under 0.75 and 1.5; 0.5 and 1 scale exactly)


@pytest.mark.parametrize("shape", CO.INJECT_SHAPES)
def test_inject_cases_round_and_their_column_sums_are_exact(shape):
    c = CO.inject_case(*shape)
    y = CO.inject_ref(c)
    s = R.f64(c["x"]) + R.f64(c["r"])
    assert bool((y != s).any()) and bool((y == s).any())
    assert bool(((s - torch.floor(s)) == 0.5).any())                          # ties to even among them
    assert R.colstats_exactness(y, CO.INJECT_UNIT) < R.LIMIT
    for rows in CO.INJECT_ROWS[shape]:
        assert c["M"] % rows == 0 and rows % 16 == 0
        st = R.colstats_ref(y, rows)
        assert st.shape == (c["M"] // rows, shape[2], 2)


def test_refusals_come_before_any_launch():
    from instructany2pix_amd import _ffi
    lib = _ffi.lib()
    p = C.c_void_p(4096)
    INVALID, SHAPE = 1, 2
    cases = [
        (INVALID, lib.ia2p_conv3x3_narrow(None, None, p, p, p, 1, 8, 8, 16, 16, 1, 0)),
        (INVALID, lib.ia2p_conv3x3_narrow(None, p, p, p, p, 1, 8, 8, 16, 16, 1, 2)),
        (SHAPE, lib.ia2p_conv3x3_narrow(None, p, p, p, p, 1, 8, 8, 24, 16, 1, 0)),            # Cin % 16
        (SHAPE, lib.ia2p_conv3x3_narrow(None, p, p, p, p, 1, 8, 8, 272, 16, 1, 0)),           # Cin > 256
        (SHAPE, lib.ia2p_conv3x3_narrow(None, p, p, p, p, 1, 8, 8, 16, 24, 1, 0)),            # Co % 16
        (SHAPE, lib.ia2p_conv3x3_narrow(None, p, p, p, p, 1, 8, 8, 16, 16, 3, 0)),            # stride
        (INVALID, lib.ia2p_conv_in_act(None, p, p, p, None, p, 1, 3, 8, 8, 16, 1)),
        (SHAPE, lib.ia2p_conv_in_act(None, p, p, p, p, p, 1, 8, 8, 8, 16, 1)),                # Cin * 9 > 64
        (INVALID, lib.ia2p_gemm_rowscale(None, p, p, p, None, p, 64, 64, 64, 16)),
        (INVALID, lib.ia2p_gemm_rowscale(None, p, p, p, C.c_void_p(4098), p, 64, 64, 64, 16)),
        (SHAPE, lib.ia2p_gemm_rowscale(None, p, p, p, p, p, 64, 64, 96, 16)),                 # K % 64
        (SHAPE, lib.ia2p_gemm_rowscale(None, p, p, p, p, p, 64, 64, 64, 24)),                 # HW does not divide M
        (INVALID, lib.ia2p_residual_add_gnstats(None, p, None, p, 64, 64, 16, None)),
        (INVALID, lib.ia2p_residual_add_gnstats(None, p, C.c_void_p(4104), p, 64, 64, 16, None)),
        (SHAPE, lib.ia2p_residual_add_gnstats(None, p, p, p, 64, 60, 16, None)),              # C % 8
        (SHAPE, lib.ia2p_residual_add_gnstats(None, p, p, p, 64, 64, 8, p)),                  # runs of 16 rows
        (SHAPE, lib.ia2p_residual_add_gnstats(None, p, p, p, 72, 64, 16, p)),                 # rows does not divide M
    ]
    for i, (want, got) in enumerate(cases):
        assert got == want, (i, want, got)
