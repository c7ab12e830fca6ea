"""The ViT, SAM and mask-decoder attention launches (`ia2p_attention_full`, `ia2p_attention_global_relpos`, `ia2p_attention_window_relpos`,
`ia2p_attention_small_head`) and the two mask launches (`ia2p_mask_morph`, `ia2p_mask_upsample_threshold`) one by one against the fp64 references of
tests/attn_ops_ref.py.

Every output must lie within the bound attn_ops_ref derives for its kernel, element by element (max(err / bound) <= 1, printed per test: pytest -s; docs/LOG.md §26
records a run); the morphology is held to the bit. Every output buffer starts as NaN (a sentinel for fp32 and uint8) between a guard region in front of it and one
behind it that must come back untouched; every launch runs twice and must give the same bits. A planted row must be the value row of its key."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 512
SENTINEL = {torch.float16: float("nan"), torch.float32: -7777.0, torch.uint8: 0x5A}
_INT = {torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
OK, SHAPE = 0, 2


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def _report(tag, worst):
    print(f"[attn-ops] {tag}: max(err / bound) {worst:.3g}")
    return worst <= 1.0


def _family(tag, r):
    print(f"[attn-ops]   {tag}: {r:.3g}")
    return r


class Out:
    """an output buffer of n elements filled with NaN / a sentinel, GUARD elements in front of it and `back` behind it"""

    def __init__(self, n, dtype=torch.float16, back=GUARD):
        self.n, self.dtype = int(n), dtype
        self.buf = torch.empty(GUARD + self.n + int(back), dtype=dtype, device=DEV)
        self.reset()

    def reset(self, init=None):
        self.buf.fill_(SENTINEL[self.dtype])
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


def _twice(tag, launch, outs, finite=True):
    """launch twice from freshly filled buffers: the status is OK, same bits, guards intact, every output written. -> the outputs (on the CPU)"""
    ffi, _ = _lib()
    bits = []
    for _ in range(2):
        for o in outs:
            o.reset()
        ffi.check(launch())
        torch.cuda.synchronize()
        bits.append([o.buf.view(_INT[o.dtype]).clone() for o in outs])
    for a, b in zip(*bits):
        assert torch.equal(a, b), f"{tag}: a second launch gives other bits"
    for o in outs:
        o.check(tag)
        if finite and o.dtype != torch.uint8:
            assert bool(torch.isfinite(o.out.float()).all()) and bool((o.out.float() != SENTINEL[torch.float32]).all()), f"{tag}: an output is not finite (or was never written)"
    return [o.out.cpu() for o in outs]


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _planted_ok(got, ref, bound, want, tag):
    """a planted row is its key's value row: |got - want| <= bound + |ref - want| (what the other keys still weigh in fp64)"""
    if want is None:
        return 0
    rows = ~torch.isnan(want)
    away = (ref - want).abs()[rows]
    assert float(away.max() if away.numel() else 0.0) < 1e-5, tag
    assert bool(((got.double() - want).abs()[rows] <= bound[rows] + away).all()), f"{tag}: a planted row is not its key's value row"
    return int(rows.sum())


# ---- ia2p_attention_full -------------------------------------------------------------------------------------------------------------------------------------------
def _full(qkv, bk, bv, T, D, tag):
    ffi, lib = _lib()
    B, heads = R.FULL_B, R.FULL_HEADS
    dq, dk, dv, o = _d(qkv), _d(bk), _d(bv), Out(B * T * heads * D)
    return _twice(tag, lambda: lib.ia2p_attention_full(ffi.current_stream(), ffi.ptr(dq), o.ptr, ffi.ptr(dk), ffi.ptr(dv), B, T, heads, D), [o])[0].reshape(B * T, heads * D)


@pytest.mark.parametrize("D", R.FULL_D)
@pytest.mark.parametrize("T,bias", R.FULL_T)
def test_attention_full(T, bias, D):
    """diffuse rows, and planted rows whose key is 0, 15, 16, T - 1 or the bias row (query i takes the (i mod n)-th of them: the bias-row queries return bias_v)"""
    worst, planted = 0.0, 0
    for family in ("diffuse", "planted"):
        tag = f"attention_full T={T}{'+bias' if bias else ''} D={D} {family}"
        qkv, bk, bv, want = R.full_case(family, T, bias, D)
        ref, bound, _ = R.full_ref(family, T, bias, D)
        got = _full(qkv, bk, bv, T, D, tag)
        worst = max(worst, _family(tag, R.ratio(got, ref, bound)))
        planted += _planted_ok(got, ref, bound, want, tag)
    assert planted > 0
    assert _report(f"attention_full T={T}{'+bias' if bias else ''} D={D}", worst)


def test_attention_full_refuses_273_keys():
    ffi, lib = _lib()
    t = torch.zeros(273 * 3 * 80, dtype=torch.half, device=DEV)
    o = Out(273 * 80)
    for D in R.FULL_D:
        assert lib.ia2p_attention_full(ffi.current_stream(), ffi.ptr(t), o.ptr, None, None, 1, 273, 1, D) == SHAPE
        assert lib.ia2p_attention_full(ffi.current_stream(), ffi.ptr(t), o.ptr, ffi.ptr(t), ffi.ptr(t), 1, 272, 1, D) == SHAPE
    torch.cuda.synchronize()
    o.check("refused")
    assert bool(torch.isnan(o.out).all())


# ---- ia2p_attention_global_relpos / ia2p_attention_window_relpos -----------------------------------------------------------------------------------------------
def _relpos(qkv, bias, rh, rw, gh, gw, D, window, tag, finite=True):
    ffi, lib = _lib()
    B, heads = R.relpos_dims(gh, gw, window)
    H = heads * D
    back = GUARD + ((-gh) % window) * gw * H if window else GUARD      # every row a pad QUERY could index behind the last image lands in the guard
    dq, db, dh, dw, o = _d(qkv), _d(bias), _d(rh), _d(rw), Out(B * gh * gw * H, back=back)
    s = ffi.current_stream()
    if window:
        launch = lambda: lib.ia2p_attention_window_relpos(s, ffi.ptr(dq), o.ptr, ffi.ptr(db), ffi.ptr(dh), ffi.ptr(dw), B, gh, gw, heads, D, window)      # noqa: E731
    else:
        launch = lambda: lib.ia2p_attention_global_relpos(s, ffi.ptr(dq), o.ptr, ffi.ptr(dh), ffi.ptr(dw), B, gh, gw, heads, D)      # noqa: E731
    return _twice(tag, launch, [o], finite)[0].reshape(B * gh * gw, H)


def _relpos_family(family, window, gh, gw, D, tag):
    qkv, bias, rh, rw, want = R.relpos_case(family, window, gh, gw, D)
    ref, bound, _ = R.relpos_ref(family, window, gh, gw, D)
    got = _relpos(qkv, bias, rh, rw, gh, gw, D, window, tag)
    return got, _family(tag, R.ratio(got, ref, bound)), _planted_ok(got, ref, bound, want, tag), want, bias


@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("grid", R.GLOBAL_GRIDS, ids=lambda g: g if isinstance(g, str) else f"{g[0]}x{g[1]}")
def test_attention_global_relpos(grid, D):
    """diffuse; planted through q . k at key 0, 63, 64, nkeys - 1; planted through the tables at (dh0, dw0) = (2, -3); the first key tile 120 below the rest.
    `thin` is the widest 3-row grid the LDS limit admits (test_global_relpos_lds_limit finds the same by asking the entry point)"""
    gh, gw = R.global_grid(grid, D)
    worst, planted, fams = 0.0, 0, [c[0] for c in R.global_cases() if c[1:] == (gh, gw, D)]
    for family in fams:
        _, r, n, _, _ = _relpos_family(family, 0, gh, gw, D, f"global_relpos {gh}x{gw} D={D} {family}")
        worst, planted = max(worst, r), planted + n
    assert planted > 0 and "diffuse" in fams and "planted" in fams
    assert _report(f"attention_global_relpos {gh}x{gw} D={D} ({', '.join(fams)})", worst)


@pytest.mark.parametrize("D", [64, 80])
def test_global_relpos_lds_limit(D):
    """the widest accepted [3, gw] grid, found by calling the entry point with a growing gw: it is the one the formula gives (and the `thin` case above runs),
    its launch returns IA2P_OK, the next one is refused"""
    ffi, lib = _lib()
    gh, top = R.THIN_GH, 260
    qkv = torch.zeros(gh * top * 3 * D, dtype=torch.half, device=DEV)
    rh, rw, o = torch.zeros(2 * gh - 1, D, dtype=torch.half, device=DEV), torch.zeros(2 * top - 1, D, dtype=torch.half, device=DEV), Out(gh * top * D)
    gw, st = 150, OK
    while gw < top:
        st = lib.ia2p_attention_global_relpos(ffi.current_stream(), ffi.ptr(qkv), o.ptr, ffi.ptr(rh), ffi.ptr(rw), 1, gh, gw + 1, 1, D)
        if st != OK:
            break
        gw += 1
    torch.cuda.synchronize()
    o.check("growing gw")
    print(f"[attn-ops] global relpos D={D}: the largest accepted 3-row grid is {gh} x {gw} (gh + gw = {gh + gw}), {R.relpos_lds_bytes(D, gh, gw)} bytes of LDS")
    assert st == SHAPE and (gh, gw) == R.thin_grid(D)
    assert lib.ia2p_attention_global_relpos(ffi.current_stream(), ffi.ptr(qkv), o.ptr, ffi.ptr(rh), ffi.ptr(rw), 1, gh, gw, 1, D) == OK
    assert lib.ia2p_attention_global_relpos(ffi.current_stream(), ffi.ptr(qkv), o.ptr, ffi.ptr(rh), ffi.ptr(rw), 1, gh, gw + 1, 1, D) == SHAPE
    torch.cuda.synchronize()


@pytest.mark.parametrize("window,gh,gw,D", R.WINDOW_CASES)
def test_attention_window_relpos(window, gh, gw, D):
    """diffuse; planted at the real keys among 0, 63, 64, nkeys - 1 of every window; the bias' k row planted: every query of a window with pad keys returns the
    bias' v row, queries of full windows do not"""
    worst, planted = 0.0, 0
    for family in ("diffuse", "planted", "pad"):
        tag = f"window_relpos w={window} {gh}x{gw} D={D} {family}"
        got, r, n, want, bias = _relpos_family(family, window, gh, gw, D, tag)
        worst, planted = max(worst, r), planted + n
        if family == "pad":
            B, heads = R.relpos_dims(gh, gw, window)
            full = torch.isnan(want).all(1)
            nfull = (gh // window) * (gw // window) * window * window * B      # the queries of full windows: none where the grid is smaller than a window on an axis
            assert int(full.sum()) == nfull and (nfull > 0) == (gh >= window and gw >= window), f"{tag}: {int(full.sum())} queries of full windows, {nfull} expected"
            bv = bias.double().reshape(3, heads * D)[2]
            assert bool(((got.double()[full] - bv).abs().max(1).values > 0.1).all()), f"{tag}: a query of a full window returns the bias' v row"
            assert n == int((~full).sum()) * heads * D
    assert planted > 0
    assert _report(f"attention_window_relpos w={window} {gh}x{gw} D={D}", worst)


@pytest.mark.parametrize("window,gh,gw,D,wy,wx", [(14, 20, 20, 80, 0, 0), (14, 20, 20, 80, 1, 1), (7, 20, 20, 64, 2, 1), (16, 32, 20, 80, 1, 1)])
def test_window_relpos_pad_isolation(window, gh, gw, D, wy, wx):
    """every real token of one window of image 0 is NaN (q, k and v): the outputs of every other window, and of image 1, keep the bits of the clean run"""
    qkv, bias, rh, rw, _ = R.relpos_case("diffuse", window, gh, gw, D)
    B, heads = R.relpos_dims(gh, gw, window)
    clean = _relpos(qkv, bias, rh, rw, gh, gw, D, window, "clean")
    idx = next(i for y, x, _, i in R.rectangles(gh, gw, window, window) if (y, x) == (wy, wx))
    bad = qkv.clone()
    bad[idx] = float("nan")
    got = _relpos(bad, bias, rh, rw, gh, gw, D, window, "one window NaN", finite=False)
    keep = torch.ones(B * gh * gw, dtype=torch.bool)
    keep[idx] = False
    assert torch.equal(got[keep].view(torch.int16), clean[keep].view(torch.int16)), "a window reads another window's tokens"
    assert bool(torch.isnan(got[~keep]).all())


# ---- ia2p_attention_small_head ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.SMALL_D)
@pytest.mark.parametrize("B,Tq,Tk,heads", R.SMALL_SHAPES)
def test_attention_small_head(B, Tq, Tk, heads, D):
    """diffuse rows, and planted rows whose key is 0, 63, 64 or Tk - 1"""
    ffi, lib = _lib()
    worst, planted = 0.0, 0
    for family in ("diffuse", "planted"):
        tag = f"small_head {B}x{Tq}x{Tk}x{heads} D={D} {family}"
        q, k, v, want = R.small_case(family, B, Tq, Tk, heads, D)
        ref, bound, _ = R.small_ref(family, B, Tq, Tk, heads, D)
        dq, dk, dv, o = _d(q), _d(k), _d(v), Out(B * Tq * heads * D)
        got = _twice(tag, lambda: lib.ia2p_attention_small_head(ffi.current_stream(), ffi.ptr(dq), ffi.ptr(dk), ffi.ptr(dv), o.ptr, B, Tq, Tk, heads, D), [o])[0].reshape(B, Tq, heads * D)
        worst = max(worst, _family(tag, R.ratio(got, ref, bound)))
        planted += _planted_ok(got, ref, bound, want, tag)
    assert planted > 0
    assert _report(f"attention_small_head B={B} Tq={Tq} Tk={Tk} heads={heads} D={D}", worst)


# ---- ia2p_mask_morph -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", R.MORPH_H)
@pytest.mark.parametrize("W", R.MORPH_W)
def test_mask_morph(W, H):
    """k = 1, 2, 7, 10 and 700 (larger than the image), erode and dilate, random masks and single-pixel masks at the corners and around column 255 / 256: equal to
    the plain filter to the bit; dst == src gives the bits of the out-of-place call"""
    ffi, lib = _lib()
    s = ffi.current_stream()
    tmp, dst, inplace = Out(H * W, torch.uint8), Out(H * W, torch.uint8), Out(H * W, torch.uint8)
    for i, m in enumerate(R.morph_masks(H, W, 10 * W + H)):
        src = torch.from_numpy(m).to(DEV)
        for k in R.MORPH_K:
            for dilate in (0, 1):
                tag = f"mask_morph {H}x{W} k={k} dilate={dilate} mask {i}"
                launch = lambda: lib.ia2p_mask_morph(s, ffi.ptr(src), dst.ptr, tmp.ptr, H, W, k, dilate)      # noqa: E731
                if i < 3:
                    got = _twice(tag, launch, [dst, tmp])[0]
                else:
                    dst.reset(), tmp.reset()
                    ffi.check(launch())
                    torch.cuda.synchronize()
                    dst.check(tag), tmp.check(tag)
                    got = dst.out.cpu()
                assert np.array_equal(got.numpy().reshape(H, W), R.morph(m, k, bool(dilate))), tag
                if i < 4:
                    inplace.reset(src)
                    tmp.reset()
                    ffi.check(lib.ia2p_mask_morph(s, inplace.ptr, inplace.ptr, tmp.ptr, H, W, k, dilate))
                    torch.cuda.synchronize()
                    inplace.check(tag), tmp.check(tag)
                    assert torch.equal(inplace.out.cpu(), got), f"{tag}: dst == src gives other bits"


# ---- ia2p_mask_upsample_threshold ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.UPSAMPLE_CASES])
def test_mask_upsample_threshold(name):
    """logits within the bound of the fp64 resize; the mask equal to ref > thr wherever the reference is farther from the threshold than its bound (at most 1 % of
    the pixels are not), at thresholds 0 and 0.37; logits only, mask only and both give the same bits"""
    ffi, lib = _lib()
    _, n, sh, sw, rows, ld, H, W = next(c for c in R.UPSAMPLE_CASES if c[0] == name)
    x = R.upsample_case(name)
    ref, bound = R.bilinear_resize(x, sh, sw, H, W)
    dx, s = x.to(DEV), ffi.current_stream()
    worst = 0.0
    for thr in R.UPSAMPLE_THR:
        tag = f"mask_upsample_threshold {name} thr={thr}"
        lo, mk, lo1, mk1 = Out(n * H * W, torch.float32), Out(n * H * W, torch.uint8), Out(n * H * W, torch.float32), Out(n * H * W, torch.uint8)
        call = lambda a, b: lib.ia2p_mask_upsample_threshold(s, ffi.ptr(dx), n, sh, sw, ld, rows * ld, H, W, thr, a, b)      # noqa: E731
        logits, mask = _twice(tag, lambda: call(lo.ptr, mk.ptr), [lo, mk])
        only_l = _twice(tag + " logits only", lambda: call(lo1.ptr, None), [lo1])[0]
        only_m = _twice(tag + " mask only", lambda: call(None, mk1.ptr), [mk1])[0]
        assert torch.equal(only_l.view(torch.int32), logits.view(torch.int32)) and torch.equal(only_m, mask), f"{tag}: one output alone gives other bits"
        worst = max(worst, R.ratio(logits.reshape(n, H, W), ref, bound))
        mask = mask.reshape(n, H, W)
        assert bool(((mask == 0) | (mask == 255)).all())
        sure = R.sure_pixels(ref, bound, thr)
        assert 1.0 - float(sure.double().mean()) <= 0.01
        assert torch.equal((mask == 255)[sure], (ref > float(np.float32(thr)))[sure]), f"{tag}: the mask is not ref > thr on a decided pixel"
    assert _report(f"mask_upsample_threshold {name}", worst)
