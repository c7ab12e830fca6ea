"""The UNet's fused attention launches -- `ia2p_attention` in its three modes (one segment; text + image tokens in one merged accumulator, folded into the last text
tile or not, resident or streamed; two generic segments), `ia2p_qproj_attention`, `ia2p_qkv_self_attention` and `ia2p_qkv_self_attention_ctx` -- against the fp64
reference of tests/unet_attn_ref.py.

Every output element must lie within the bound unet_attn_ref derives from csrc/attention_core.h (max(err / bound) <= 1, printed per test: pytest -s; docs/LOG.md §37
records a run). A planted row of a one-segment launch must be its key's fp16 value row to the bit. Every launch runs twice into NaN-filled buffers between guard
regions and must give the same bits; with ldo > heads 64 the columns between one row's heads and the next row keep their bits. The fused launches project with an
identity weight, so Q (or Q | K | V) is X to the bit, the same reference applies, and their outputs are also the stand-alone launch's bits."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_attn_ref as R  # noqa: E402
from test_unet_ops_gpu import Out, _d, _p, _twice  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_, H_ = R.B_, R.HEADS


@pytest.fixture(scope="module")
def L():
    from instructany2pix_amd import _ffi
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib = _ffi.lib()
    assert lib.ia2p_device_is_gfx950() == 1
    yield lib
    lib.ia2p_debug_set_attn_fold(-1)


def _stream():
    from instructany2pix_amd import _ffi
    return _ffi.current_stream()


def _at(t, elems):
    return C.c_void_p(t.data_ptr() + 2 * elems)


def _report(tag, worst):
    print(f"[unet-attn] {tag}: max(err / bound) {worst:.3g}")
    assert worst <= 1.0, f"{tag}: an output leaves its bound, max(err / bound) {worst:.3g}"


def _segs(c):
    """the key segments of a case on the device, K | V side by side per row as the executor keeps them -> (keep-alive tensors, the entry point's segment arguments)"""
    _, B, heads, Nq, n0, n1, w0, w1 = c
    Cc = heads * 64
    _, k0, v0, k1, v1, _ = R.case(*c)
    kv0 = _d(torch.cat([k0, v0], -1))
    kv1 = _d(torch.cat([k1, v1], -1)) if n1 else None
    return (kv0, kv1), (2 if n1 else 1, _p(kv0), _at(kv0, Cc), 2 * Cc, n0, w0, _p(kv1), None if kv1 is None else _at(kv1, Cc), 2 * Cc if n1 else 0, n1, w1)


def _attention(L, c, tag, packed=False, pad=0):
    """ia2p_attention on a case, twice -> out [B, Nq, heads 64] on the CPU. packed: the self-attention layout, Q | K | V in one tensor with ldq = ld = 3 C"""
    _, B, heads, Nq, n0, n1, w0, w1 = c
    Cc = heads * 64
    ldo = Cc + pad
    q = R.case(*c)[0]
    if packed:
        _, k0, v0 = R.case(*c)[:3]
        qkv = _d(torch.cat([q, k0, v0], -1))
        keep, args = qkv, (_p(qkv), 3 * Cc, 1, _at(qkv, Cc), _at(qkv, 2 * Cc), 3 * Cc, n0, w0, None, None, 0, 0, 0.0)
    else:
        dq = _d(q)
        keep, segs = _segs(c)
        keep, args = (keep, dq), (_p(dq), Cc) + segs
    o = Out(B * Nq * ldo)
    s = _stream()
    got = _twice(tag, lambda: L.ia2p_attention(s, args[0], args[1], o.ptr, ldo, B, heads, Nq, *args[2:]), [o], partly=(o,) if pad else ())[0].reshape(B, Nq, ldo)
    if pad:
        nan = torch.full((1,), float("nan"), dtype=torch.half).view(torch.int16)
        assert bool((got[..., Cc:].contiguous().view(torch.int16) == nan).all()), f"{tag}: wrote between one row's heads and the next row"
        assert bool(torch.isfinite(got[..., :Cc].float()).all()), f"{tag}: an output is not finite (or was never written)"
    del keep
    return got[..., :Cc].contiguous()


def _hold(c, got, tag):
    """every element within its bound; a planted row is its keys' value rows (one segment of weight 1: to the bit) -> max(err / bound)"""
    ref, bound, _ = R.ref(*c)
    want = R.case(*c)[5]
    r = R.ratio(got, ref, bound)
    print(f"[unet-attn]   {tag}: {r:.3g}")
    if want is not None:
        if not c[5] and c[6] == 1.0:
            assert torch.equal(got.double(), want), f"{tag}: a planted row is not its key's value row to the bit"
        else:
            assert bool(((got.double() - want).abs() <= bound + (ref - want).abs()).all()), f"{tag}: a planted row is not w0 v_a + w1 v_b"
    return r


def _families(L, shape, tag, outs=None, **kw):
    worst = 0.0
    for family in R.FAMILIES:
        c = (family,) + shape
        got = _attention(L, c, f"{tag} {family}", **kw)
        worst = max(worst, _hold(c, got, f"{tag} {family}"))
        if outs is not None:
            outs.append(got)
    return worst


# ---- ia2p_attention ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.SELF_N)
def test_attention_one_segment_self_layout(L, N):
    """MODE 0, Nq = nkeys from one packed qkv tensor: every DMA stage edge (128 keys a stage, two buffers) and every partial last tile"""
    tag = f"attention self N={N}"
    _report(tag, _families(L, (B_, H_, N, N, 0, 1.0, 0.0), tag, packed=True))


@pytest.mark.parametrize("B,heads,Nq,nkeys", [(B_, H_) + s for s in R.CROSS] + [R.CROSS_ONE_WG, R.CROSS_NINE_WG])
def test_attention_one_segment_query_blocks(L, B, heads, Nq, nkeys):
    """MODE 0, Nq != nkeys: one to three query blocks of 128, the last one partial; 1, 6, 9, 12 and 18 workgroups under the XCD remap"""
    tag = f"attention B={B} heads={heads} Nq={Nq} nkeys={nkeys}"
    _report(tag, _families(L, (B, heads, Nq, nkeys, 0, 1.0, 0.0), tag))


@pytest.mark.parametrize("Lt,Li,w0,w1", R.TWO)
def test_attention_two_segments(L, Lt, Li, w0, w1):
    """MODE 1 (resident and folded, resident and not, streamed) and MODE 2. A fold-eligible case runs with the image-token keys folded into the last text tile and
    with a tile of their own, each form held to the bound on its own"""
    shape = (B_, H_, R.TWO_NQ, Lt, Li, float(w0), float(w1))
    folds = R.mode(Li, w0) == 1 and R.fold_ok(Lt, Li) and -(-Lt // 64) + -(-Li // 64) <= 4
    assert folds == ((Lt, Li, w0, w1) in R.FOLDED)
    worst, outs = 0.0, {1: [], 0: [], -1: []}
    try:
        for fold in ((1, 0) if folds else (-1,)):
            L.ia2p_debug_set_attn_fold(fold)
            tag = f"attention two segments ({Lt}, {Li}, {w0}, {w1}) mode {R.mode(Li, w0)}" + (f" fold {fold}" if folds else "")
            worst = max(worst, _families(L, shape, tag, outs[fold]))
    finally:
        L.ia2p_debug_set_attn_fold(-1)
    if folds:      # (the two forms sum in another order: how many outputs got other bits is printed, test_ops_gpu.py holds them to one ulp of each other)
        a, b = torch.stack(outs[1]), torch.stack(outs[0])
        print(f"[unet-attn]   folded against unfolded: {float((a != b).double().mean()):.3%} of the outputs differ")
    _report(f"attention two segments ({Lt}, {Li}, {w0}, {w1})", worst)


@pytest.mark.parametrize("pad", R.LAYOUT_PADS)
def test_attention_output_rows_wider_than_the_heads(L, pad):
    """ldo = heads 64 + 8 and + 64 into a buffer of NaN: the 128-byte lines of attn_store_o leave the columns behind a row's heads and both guards alone, and the
    clamped rows q >= Nq of the last query block are discarded"""
    worst = 0.0
    for shape in [s + (0, 1.0, 0.0) for s in R.LAYOUT_ONE] + [(B_, H_, R.TWO_NQ, lt, li, float(a), float(b)) for lt, li, a, b in R.LAYOUT_TWO]:
        worst = max(worst, _families(L, shape, f"attention ldo = heads 64 + {pad} {shape}", pad=pad))
    _report(f"attention ldo = heads 64 + {pad}", worst)


# ---- ia2p_qproj_attention ------------------------------------------------------------------------------------------------------------------------------------------
def _qproj(L, c, tag):
    """ia2p_qproj_attention with Wq = the identity and no bias (Q = X to the bit), twice -> out [B, Nq, heads 64] on the CPU"""
    _, B, heads, Nq, n0, n1, w0, w1 = c
    Cc = heads * 64
    X, Wq = _d(R.case(*c)[0].reshape(B * Nq, Cc)), torch.eye(Cc, dtype=torch.half, device=DEV)
    keep, segs = _segs(c)
    o = Out(B * Nq * Cc)
    s = _stream()
    got = _twice(tag, lambda: L.ia2p_qproj_attention(s, _p(X), _p(Wq), None, None, o.ptr, Cc, B, heads, Nq, Cc, *segs), [o])[0].reshape(B, Nq, Cc)
    del keep
    return got


QPROJ = [(R.QPROJ_NQ[0], n, 0, 1.0, 0.0) for n in R.QPROJ_ONE] + [(R.QPROJ_NQ[0],) + tuple(c) for c in R.QPROJ_TWO] + [(R.QPROJ_NQ[1],) + tuple(c) for c in R.QPROJ_384]


@pytest.mark.parametrize("Nq,Lt,Li,w0,w1", QPROJ)
def test_qproj_attention(L, Nq, Lt, Li, w0, w1):
    """the fused to_q + attention launch against the fp64 reference directly, and to the bits of ia2p_attention on Q = X. One segment of 13 .. 192 keys is the only way
    to the single live half (nkh == 1) and the PRE staging in MODE 0; the two-segment cases are those of at most three key tiles"""
    shape = (B_, H_, Nq, Lt, Li, float(w0), float(w1))
    folds = R.mode(Li, w0) == 1 and R.fold_ok(Lt, Li)
    worst = 0.0
    try:
        for fold in ((1, 0) if folds else (-1,)):
            L.ia2p_debug_set_attn_fold(fold)
            for family in R.FAMILIES:
                c = (family,) + shape
                tag = f"qproj_attention Nq={Nq} ({Lt}, {Li}, {w0}, {w1}) {family}" + (f" fold {fold}" if folds else "")
                got = _qproj(L, c, tag)
                worst = max(worst, _hold(c, got, tag))
                alone = _attention(L, c, tag + " stand-alone")
                assert torch.equal(got.view(torch.int16), alone.view(torch.int16)), f"{tag}: not the bits of ia2p_attention on Q = X"
    finally:
        L.ia2p_debug_set_attn_fold(-1)
    _report(f"qproj_attention Nq={Nq} ({Lt}, {Li}, {w0}, {w1})", worst)


# ---- ia2p_qkv_self_attention (_ctx) --------------------------------------------------------------------------------------------------------------------------------
def _sattn_inputs(c):
    _, B, heads, N = c[:4]
    q, k0, v0 = R.case(*c)[:3]
    return _d(torch.cat([q, k0, v0], -1).reshape(B * N, 3 * heads * 64)), torch.eye(3 * heads * 64, dtype=torch.half, device=DEV)


def test_qkv_self_attention(L):
    """the fused QKV + self-attention launch at its fixed 256 tokens with Wqkv = the identity ([Q | K | V] = X to the bit): the four families within the bound, and the
    bits of ia2p_attention on the same qkv"""
    s = _stream()
    Cc, worst = H_ * 64, 0.0
    for family in R.FAMILIES:
        c = (family, B_, H_, R.SATTN_N, R.SATTN_N, 0, 1.0, 0.0)
        tag = f"qkv_self_attention {family}"
        X, W = _sattn_inputs(c)
        o = Out(B_ * R.SATTN_N * Cc)
        got = _twice(tag, lambda: L.ia2p_qkv_self_attention(s, _p(X), _p(W), None, None, o.ptr, Cc, B_, H_, 3 * Cc), [o])[0].reshape(B_, R.SATTN_N, Cc)
        worst = max(worst, _hold(c, got, tag))
        alone = _attention(L, c, tag + " stand-alone", packed=True)
        assert torch.equal(got.view(torch.int16), alone.view(torch.int16)), f"{tag}: not the bits of ia2p_attention on the same qkv"
    _report("qkv_self_attention", worst)


def test_qkv_self_attention_ctx(L):
    """the same launch carrying a context K/V slice (77 text + 4 image-token rows): O keeps its bits, the K/V columns are the stand-alone projection's, and the
    columns around them in the wider buffer are left alone"""
    s = _stream()
    c = ("diffuse", B_, H_, R.SATTN_N, R.SATTN_N, 0, 1.0, 0.0)
    Cc, N, ctxd, Lc, Li = H_ * 64, 2 * H_ * 64, 128, 81, 4
    Lt, ldkv, col = Lc - Li, 2 * H_ * 64 + 128, 64
    X, W = _sattn_inputs(c)
    g = R.gen(81)
    ctx = _d(R._rn(g, B_, Lc, ctxd).half())
    Wt, Wi = _d((R._rn(g, N, ctxd) * ctxd ** -0.5).half()), _d((R._rn(g, N, ctxd) * ctxd ** -0.5).half())
    o, o1, kt, ki = Out(B_ * R.SATTN_N * Cc), Out(B_ * R.SATTN_N * Cc), Out(B_ * Lt * ldkv), Out(B_ * Li * ldkv)
    plain = _twice("qkv_self_attention", lambda: L.ia2p_qkv_self_attention(s, _p(X), _p(W), None, None, o.ptr, Cc, B_, H_, 3 * Cc), [o])[0]
    went = C.c_int(-1)
    at = lambda out: C.c_void_p(out.ptr.value + 2 * col)      # noqa: E731
    got, kv_t, kv_i = _twice("qkv_self_attention_ctx", lambda: L.ia2p_qkv_self_attention_ctx(s, _p(X), _p(W), None, None, o1.ptr, Cc, B_, H_, 3 * Cc, _p(ctx), Lc, Li, ctxd, _p(Wt), _p(Wi),
                                                                                            at(kt), at(ki), ldkv, N, C.addressof(went)), [o1, kt, ki], partly=(kt, ki))
    assert went.value in (0, 1)
    assert torch.equal(got.view(torch.int16), plain.view(torch.int16)), "the launch with context tiles gives other O bits"
    _report(f"qkv_self_attention_ctx (in_launch {went.value})", _hold(c, got.reshape(B_, R.SATTN_N, Cc), "qkv_self_attention_ctx diffuse"))
    for kv, rows, Wp in ((kv_t.reshape(B_ * Lt, ldkv), ctx[:, :Lt].reshape(B_ * Lt, ctxd).contiguous(), Wt), (kv_i.reshape(B_ * Li, ldkv), ctx[:, Lt:].reshape(B_ * Li, ctxd).contiguous(), Wi)):
        M = rows.shape[0]
        ref = Out(M * N)
        want = _twice("context projection", lambda: L.ia2p_gemm_ex(s, _p(rows), _p(Wp), None, None, ref.ptr, M, N, ctxd, 0, None, None, None, 1, None), [ref])[0].reshape(M, N)
        assert torch.equal(kv[:, col:col + N].contiguous().view(torch.int16), want.view(torch.int16)), "K/V columns are not the stand-alone projection's bits"
        assert bool(torch.isnan(kv[:, :col]).all()) and bool(torch.isnan(kv[:, col + N:]).all()), "wrote outside the layer's K/V columns"
