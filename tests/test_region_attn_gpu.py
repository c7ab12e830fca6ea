"""`ia2p_attention_regions` (csrc/attention_regions.hip) against the fp64 reference of tests/region_attn_ref.py, element by element, and `ia2p_region_levels` to the bit.

Every output element must lie within the bound region_attn_ref derives from the kernel's code (max(err / bound) <= 1, printed per test: pytest -s). Every launch runs
twice into NaN-filled buffers between guard regions and must give the same bits. The shapes are region_attn_ref.SHAPES: one Nq sweep at n0 = 77, G = 3, one G sweep at
Nq = 160, one n0 sweep and the five mask kinds at the base shape, each for the four Q / K families of unet_attn_ref.FAMILIES.

Properties on the same inputs: locality and padding on the bits, the two formulas the regional one degenerates to (one group with m == 1: two segments; every mask
zero: one segment) against the bounds of unet_attn_ref.unet_attention, and the refusals that need a device pointer's alignment only."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_attn_ref as R  # noqa: E402
import unet_attn_ref as UA  # noqa: E402
from test_unet_ops_gpu import Out, _d, _p, _twice  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    from instructany2pix_amd import _ffi
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = _ffi.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    return lib


def _stream():
    from instructany2pix_amd import _ffi
    return _ffi.current_stream()


def _at(t, elems):
    return C.c_void_p(t.data_ptr() + 2 * elems)


def _report(tag, worst):
    print(f"[region-attn] {tag}: max(err / bound) {worst:.3g}")
    assert worst <= 1.0, f"{tag}: an output leaves its bound, max(err / bound) {worst:.3g}"


def _launch(L, q, k0, v0, k1, v1, m, w0, s, heads, tag, per_row=True):
    """ia2p_attention_regions, twice -> out [B, Nq, heads 64] on the CPU. K | V side by side per row, as the executor keeps them. per_row: s[b] through w1_b, else s[0] as w1"""
    B, Nq, Cc = q.shape
    G, n0 = m.shape[1], k0.shape[1]
    dq, kv0, kv1, dm = _d(q), _d(torch.cat([k0, v0], -1)), _d(torch.cat([k1, v1], -1)), _d(m)
    sb = torch.tensor(list(s), dtype=torch.float32, device=DEV) if per_row else None
    o = Out(B * Nq * Cc)
    st = _stream()
    got = _twice(tag, lambda: L.ia2p_attention_regions(st, _p(dq), Cc, o.ptr, Cc, B, heads, Nq, 2, _p(kv0), _at(kv0, Cc), 2 * Cc, n0, w0,
                                                      _p(kv1), _at(kv1, Cc), 2 * Cc, 4 * G, float(s[0]), _p(dm), G, _p(sb)), [o])[0]
    return got.reshape(B, Nq, Cc)


def _run(L, c, tag):
    _, B, heads, Nq, n0, G, kind, w0 = c
    q, k0, v0, k1, v1, m = R.case(*c)
    return _launch(L, q, k0, v0, k1, v1, m, w0, R.S_B[:B], heads, tag)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "B{}-h{}-Nq{}-n0_{}-G{}-{}-w0_{}".format(*s))
def test_attention_regions_meets_the_bound(L, shape):
    worst = 0.0
    for family in R.FAMILIES:
        c = (family,) + shape
        got = _run(L, c, f"regions {c}")
        ref, bound, _ = R.ref(*c)
        r = R.ratio(got, ref, bound)
        print(f"[region-attn]   {family}: {r:.3g}")
        worst = max(worst, r)
    _report(f"regions {shape}", worst)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("kind", ["rect", "zero"])
def test_locality_on_the_bits(L, kind):
    """other finite K and V rows for group g: every output at queries with m[b, g, q] == 0 keeps its bits"""
    B, heads, Nq, n0, G = R.BASE
    for family in ("diffuse", "planted"):
        q, k0, v0, k1, v1, m = R.case(family, B, heads, Nq, n0, G, kind, 1.0)
        base = _launch(L, q, k0, v0, k1, v1, m, 1.0, R.S_B, heads, f"locality {family} base")
        gen = torch.Generator().manual_seed(11)
        for g in range(G):
            k1b, v1b = k1.clone(), v1.clone()
            k1b[:, 4 * g:4 * g + 4] = (3.0 * torch.randn(B, 4, heads * 64, generator=gen)).half()
            v1b[:, 4 * g:4 * g + 4] = (100.0 * torch.randn(B, 4, heads * 64, generator=gen)).half()
            got = _launch(L, q, k0, v0, k1b, v1b, m, 1.0, R.S_B, heads, f"locality {family} group {g}")
            off = (m[:, g] == 0).reshape(B, Nq, 1).expand_as(got)
            assert bool(off.any())
            assert torch.equal(_bits(got)[off], _bits(base)[off]), f"{family}: group {g} moves outputs where its mask is 0"
            if not bool(off.all()):      # (the all-zero group of `zero` has no query left)
                assert not torch.equal(_bits(got)[~off], _bits(base)[~off]), f"{family}: group {g} has no effect where its mask is not 0"


@pytest.mark.parametrize("G,pad", [(3, 1), (3, 6), (8, 1), (1, 15)])
def test_padding_on_the_bits(L, G, pad):
    """all-zero groups with arbitrary finite tokens behind the case's own: the same bits (G + pad crosses the half-tile at 8 -> 9 and fills the tile at 16)"""
    B, heads, Nq, n0, _ = R.BASE
    gen = torch.Generator().manual_seed(G * 17 + pad)
    for family in ("diffuse", "peaked"):
        q, k0, v0, k1, v1, m = R.case(family, B, heads, Nq, n0, G, "ramp", 1.0)
        base = _launch(L, q, k0, v0, k1, v1, m, 1.0, R.S_B, heads, f"padding {family} base")
        k1p = torch.cat([k1, (2.0 * torch.randn(B, 4 * pad, heads * 64, generator=gen)).half()], 1)
        v1p = torch.cat([v1, (50.0 * torch.randn(B, 4 * pad, heads * 64, generator=gen)).half()], 1)
        mp = torch.cat([m, torch.zeros(B, pad, Nq, dtype=torch.half)], 1)
        got = _launch(L, q, k0, v0, k1p, v1p, mp, 1.0, R.S_B, heads, f"padding {family} G {G} + {pad}")
        assert torch.equal(_bits(got), _bits(base)), f"{family}: {pad} all-zero groups behind {G} move an output"


@pytest.mark.parametrize("n0,w0,s", [(77, 1.0, 1.0), (64, 0.5, 1.3), (120, 1.0, 0.7)])
def test_one_group_all_one_is_the_two_segment_formula(L, n0, w0, s):
    """G = 1, m == 1: the bound of unet_attn_ref.unet_attention with n1 = 4 and w1 = s"""
    B, heads, Nq = 2, 3, UA.TWO_NQ
    worst = 0.0
    for family in UA.FAMILIES:
        c = (family, B, heads, Nq, n0, 4, w0, s)
        q, k0, v0, k1, v1, _ = UA.case(*c)
        ref, bound, _ = UA.ref(*c)
        got = _launch(L, q, k0, v0, k1, v1, torch.ones(B, 1, Nq, dtype=torch.half), w0, (s, s), heads, f"one group {c}", per_row=False)
        worst = max(worst, UA.ratio(got, ref, bound))
    _report(f"one group, m == 1, n0={n0} w0={w0} s={s}", worst)


@pytest.mark.parametrize("n0,G", [(77, 3), (64, 16)])
def test_every_mask_zero_is_the_one_segment_formula(L, n0, G):
    B, heads, Nq = 2, 3, UA.TWO_NQ
    worst = 0.0
    for family in UA.FAMILIES:
        c1 = (family, B, heads, Nq, n0, 0, 1.0, 0.0)
        ref, bound, _ = UA.ref(*c1)
        q, k0, v0, _, _, _ = UA.case(*c1)
        k1 = torch.randn(B, 4 * G, heads * 64, generator=torch.Generator().manual_seed(G)).half()
        got = _launch(L, q, k0, v0, k1, 1 + k1, torch.zeros(B, G, Nq, dtype=torch.half), 1.0, R.S_B, heads, f"all zero {c1} G={G}")
        worst = max(worst, UA.ratio(got, ref, bound))
    _report(f"every mask zero, n0={n0} G={G}", worst)


@pytest.mark.parametrize("kind", ["binary", "soft"])
def test_region_levels_to_the_bit(L, kind):
    for h, w in R.LEVEL_HW:
        m = R.levels_case(kind, h, w)
        dm = _d(m)
        for f in R.LEVEL_F:
            n = R.LEVEL_B * R.LEVEL_G * (h // f) * (w // f)
            o = Out(n)
            st = _stream()
            got = _twice(f"levels {kind} {h}x{w} f={f}", lambda: L.ia2p_region_levels(st, _p(dm), o.ptr, R.LEVEL_B, R.LEVEL_G, h, w, f), [o])[0]
            want = R.levels(m, f).reshape(-1)
            assert torch.equal(got.double(), want), f"levels {kind} {h}x{w} f={f}: not the float64 mean rounded once"


def test_refusals(L):
    """the refusals of the two entry points with real device pointers: nothing is launched, the output keeps its NaN"""
    from instructany2pix_amd import _ffi
    INVALID, SHAPE = 1, 2
    B, heads, Nq, n0, G = 1, 1, 16, 8, 2
    t = torch.zeros(4096, dtype=torch.half, device=DEV)
    o = Out(B * Nq * 64)
    p, st = _p(t), _stream()

    def att(Q=p, ldq=64, O=None, ldo=64, nseg=2, K0=p, V0=p, ld0=128, K1=p, V1=p, ld1=128, n1=4 * G, w0=1.0, rw=p, g=G):
        return L.ia2p_attention_regions(st, Q, ldq, o.ptr if O is None else O, ldo, B, heads, Nq, nseg, K0, V0, ld0, n0, w0, K1, V1, ld1, n1, 1.0, rw, g, None)

    lev = lambda m=p, out=None, h=8, w=8, f=2: L.ia2p_region_levels(st, m, o.ptr if out is None else out, 1, 2, h, w, f)      # noqa: E731
    cases = [(lambda: att(Q=C.c_void_p(0)), INVALID), (lambda: att(K0=None), INVALID), (lambda: att(V0=None), INVALID), (lambda: att(K1=None), INVALID),
             (lambda: att(V1=None), INVALID), (lambda: att(rw=None), INVALID), (lambda: att(w0=0.0), INVALID), (lambda: att(nseg=1), INVALID),
             (lambda: att(g=0, n1=0), SHAPE), (lambda: att(g=17, n1=68), SHAPE), (lambda: att(n1=4 * G + 4), SHAPE), (lambda: att(n1=4 * G - 1), SHAPE),
             (lambda: att(ldq=68), SHAPE), (lambda: att(ldo=68), SHAPE), (lambda: att(ld0=132), SHAPE), (lambda: att(ld1=132), SHAPE),
             (lambda: lev(m=None), INVALID), (lambda: lev(f=3), INVALID), (lambda: lev(f=16), INVALID), (lambda: lev(f=0), INVALID),
             (lambda: lev(h=9, f=2), SHAPE), (lambda: lev(w=10, f=4), SHAPE)]
    for i, (call, want) in enumerate(cases):
        got = call()
        assert got == want, f"case {i}: status {got}, expected {want}"
        assert L.ia2p_last_error(None), f"case {i}: no message"
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.out).all()), "a refused call wrote its output"
    o.check("refusals")
    assert _ffi.IA2P_OK == att() and _ffi.IA2P_OK == lev()
    torch.cuda.synchronize()
