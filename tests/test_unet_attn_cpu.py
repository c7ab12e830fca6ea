"""The reference of tests/unet_attn_ref.py against torch's own attention in fp64 (a wrong reference cannot bless a wrong kernel); the two conditions under which a
model may stand in a bound (the native exponential and the 2 u per MFMA addition: a tenth of the bound each, for every case the GPU tests launch); the planted rows;
and the part that shows test_unet_attn_gpu.py would fail on a subtly wrong kernel: each fault a rewrite of attention_core.h could plant is applied to the fp64
reference and must leave the bound, max(err / bound) > 1, at a named case of the GPU lists. Last, the host-side refusals of the four entry points (none reaches a
HIP call)."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_attn_ref as R  # noqa: E402

B_, H_ = R.B_, R.HEADS
SELF = lambda family, n: (family, B_, H_, n, n, 0, 1.0, 0.0)      # noqa: E731
TWO = lambda family, lt, li, w0, w1: (family, B_, H_, R.TWO_NQ, lt, li, float(w0), float(w1))      # noqa: E731


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _split(c):
    """the case's tensors per (image, head) in fp64: q, k0, v0, k1, v1 [G, n, 64]"""
    heads = c[2]
    return [None if t is None else R._heads(t, heads) for t in R.case(*c)[:5]]


def _join(c, o):
    _, B, heads, Nq = c[:4]
    return o.reshape(B, heads, Nq, 64).transpose(1, 2).reshape(B, Nq, heads * 64)


def _sm(q, k, v):
    return torch.softmax((q @ k.transpose(1, 2)) * 0.125, -1) @ v


def _worst(c, out):
    """max(err / bound) of an fp64 output against the case's reference: what the GPU test would print for a kernel that computed `out`"""
    ref, bound, _ = R.ref(*c)
    return float(((out - ref).abs() / bound).max())


# ---- the reference is right ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [SELF("diffuse", 65), SELF("ramp", 257), ("peaked", B_, H_, 160, 96, 0, 1.0, 0.0), TWO("diffuse", 77, 4, 0.5, 1.3), TWO("peaked", 96, 32, 0.75, 1),
                               TWO("ramp", 300, 4, 1, 0.9), TWO("diffuse", 300, 100, 0.5, 0.5), TWO("diffuse", 77, 4, 0, 1)], ids=str)
def test_reference_is_two_sdpa_calls(c):
    _, B, heads, Nq, n0, n1, w0, w1 = c
    sp = lambda t: t.double().reshape(B, -1, heads, 64).transpose(1, 2)      # noqa: E731
    q, k0, v0, k1, v1, _ = R.case(*c)
    want = float(torch.tensor(w0, dtype=torch.float32)) * F.scaled_dot_product_attention(sp(q), sp(k0), sp(v0))
    if n1:
        want = want + float(torch.tensor(w1, dtype=torch.float32)) * F.scaled_dot_product_attention(sp(q), sp(k1), sp(v1))
    got = R.ref(*c)[0]
    want = want.transpose(1, 2).reshape(B, Nq, heads * 64)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_case_lists_reach_what_they_are_for():
    """the lists hold what the kernel's branches need: the mode and the fold eligibility of every two-segment case, workgroup counts that are no multiple of 8"""
    assert all(R.mode(li, w0) == 1 and R.fold_ok(lt, li) and -(-lt // 64) + -(-li // 64) <= 4 for lt, li, w0, _ in R.FOLDED)
    assert all(R.mode(li, w0) == 1 and not R.fold_ok(lt, li) and -(-lt // 64) + -(-li // 64) <= 4 for lt, li, w0, _ in R.NOT_FOLDED)
    assert all(R.mode(li, w0) == 1 and -(-lt // 64) + -(-li // 64) > 4 for lt, li, w0, _ in R.STREAMED)
    assert all(R.mode(li, w0) == 2 for lt, li, w0, _ in R.MODE2)
    nwg = {(B, heads, Nq): -(-Nq // 128) * heads * B for B, heads, Nq, *_ in R.shapes()}
    assert [k for k, n in nwg.items() if n % 8 == 0] == [(B_, H_, 385)]      # four query blocks at B = 2: a multiple of 8 whatever the heads
    assert 1 in nwg.values() and 9 in nwg.values() and max(nwg.values()) > 24
    assert len(R.QPROJ_TWO) >= 10 and all(R.resident3(n, 0) for n in R.QPROJ_ONE)


def test_ramp_rises_in_every_tile():
    """the ramp family does what it is for: the running maximum of every row rises in every full 64-key tile (a last tile of one key may stay below)"""
    for n in (129, 257, 320, 513):
        q, k0 = _split(SELF("ramp", n))[:2]
        s = q @ k0.transpose(1, 2)
        tm = s[..., :n // 64 * 64].reshape(*s.shape[:-1], n // 64, 64).max(-1).values
        assert bool((tm[..., 1:] > tm[..., :-1] + 4.0).all())      # raw scores: 8 x the natural-log rise of 1.5 per tile, less the noise


# ---- the two models stay below a tenth of every bound, and every planted row is its key's value row --------------------------------------------------------
def test_shares_and_planted_rows():
    worst, planted = {f: (0.0, 0.0) for f in R.FAMILIES}, 0
    for c in R.all_cases():
        ref, bound, shares = R.ref(*c)
        worst[c[0]] = (max(worst[c[0]][0], shares[0]), max(worst[c[0]][1], shares[1]))
        assert bool(torch.isfinite(ref).all()) and bool((bound > 0).all()), c
        want = R.case(*c)[5]
        assert (want is not None) == (c[0] == "planted")
        if want is not None:
            assert bool(((ref - want).abs() <= bound).all()), f"{c}: the reference of a planted row is not its keys' value rows"
            assert float((ref - want).abs().max()) < 1e-5, c
            planted += want.numel()
    for f, (e, m) in worst.items():
        print(f"[unet-attn] {f}: largest share of the exponential / MFMA model in a bound {e:.4f} / {m:.4f}")
    assert max(max(v) for v in worst.values()) <= 0.1 and planted > 0


def test_planted_single_segment_rows_need_no_bound():
    """one segment of weight 1: the planted key's fp16 probability is 1, every other one rounds to 0: the output is the key's value row to the bit, and every
    edge key is planted in some row"""
    for n in (1, 33, 129, 513):
        c = SELF("planted", n)
        q, k0 = _split(c)[:2]
        s = (q @ k0.transpose(1, 2)) * 0.125
        top2 = s.topk(min(2, n), -1).values
        assert n == 1 or float((top2[..., 0] - top2[..., 1]).min()) >= 28.0
        assert sorted(set(s.argmax(-1).reshape(-1).tolist())) == R.edges(n)


# ---- the bound is sharp enough: planted faults ---------------------------------------------------------------------------------------------------------------
def _caught(tag, c, out):
    r = _worst(c, _join(c, out))
    print(f"[unet-attn] fault `{tag}` at {c}: max(err / bound) {r:.3g}")
    assert r > 1.0, f"{tag} at {c} stays within the bound ({r:.3g}): the GPU test would not notice it"


@pytest.mark.parametrize("n", [513, 129])
def test_fault_masked_key_leaks(n):
    """one key past the end of the last partial tile is not masked: the staging supplies a copy of the last key, whose weight doubles"""
    c = SELF("diffuse", n)
    q, k0, v0, _, _ = _split(c)
    _caught("a masked key leaks", c, _sm(q, torch.cat([k0, k0[:, -1:]], 1), torch.cat([v0, v0[:, -1:]], 1)))


def test_fault_w0_dropped_from_the_image_token_factor():
    """ci = w1 l_text / l_ip: the common w0 / l_text then leaves w0 w1 ip"""
    for c in (TWO("diffuse", 77, 4, 0.5, 1.3), TWO("planted", 13, 4, 2, 0.9)):
        q, k0, v0, k1, v1 = _split(c)
        w0, w1 = (float(torch.tensor(w, dtype=torch.float32)) for w in c[6:])
        _caught("w0 dropped from ci", c, w0 * _sm(q, k0, v0) + w0 * w1 * _sm(q, k1, v1))


def test_fault_w0_dropped_from_the_final_scale():
    """o / l_text without w0: text + (w1 / w0) ip"""
    for c in (TWO("diffuse", 77, 4, 0.5, 1.3), TWO("diffuse", 96, 32, 0.75, 1)):
        q, k0, v0, k1, v1 = _split(c)
        w0, w1 = (float(torch.tensor(w, dtype=torch.float32)) for w in c[6:])
        _caught("w0 dropped from the final scale", c, _sm(q, k0, v0) + w1 / w0 * _sm(q, k1, v1))


def test_fault_one_softmax_over_both_segments():
    c = TWO("diffuse", 77, 4, 1, 1)
    q, k0, v0, k1, v1 = _split(c)
    s = torch.cat([q @ k0.transpose(1, 2), q @ k1.transpose(1, 2)], -1) * 0.125
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    _caught("one softmax over text and image keys", c, (e / e.sum(-1, keepdim=True)) @ torch.cat([v0, v1], 1))


@pytest.mark.parametrize("lt,li", [(77, 4), (28, 4)])
def test_fault_fold_boundary_off_by_one(lt, li):
    """the key-index mask of the merged tile one key off, either way"""
    c = TWO("diffuse", lt, li, 1, 1)
    q, k0, v0, k1, v1 = _split(c)
    _caught("the first image-token key counted as text", c, _sm(q, torch.cat([k0, k1[:, :1]], 1), torch.cat([v0, v1[:, :1]], 1)) + _sm(q, k1[:, 1:], v1[:, 1:]))
    _caught("the last text key counted as image", c, _sm(q, k0[:, :-1], v0[:, :-1]) + _sm(q, torch.cat([k0[:, -1:], k1], 1), torch.cat([v0[:, -1:], v1], 1)))


def _online(q, k, v, skip=None):
    """the kernel's online softmax over 64-key tiles in fp64; `skip`: the tile whose rescale of o and l is left out"""
    s = (q @ k.transpose(1, 2)) * 0.125
    m = torch.full_like(s[..., :1], -float("inf"))
    l, o = torch.zeros_like(m), torch.zeros(*s.shape[:-1], 64, dtype=torch.float64)
    for t in range(-(-s.shape[-1] // 64)):
        st = s[..., 64 * t:64 * t + 64]
        mn = torch.maximum(m, st.max(-1, keepdim=True).values)
        alpha = torch.ones_like(m) if t == skip else torch.exp(m - mn)
        p = torch.exp(st - mn)
        l, o, m = l * alpha + p.sum(-1, keepdim=True), o * alpha + p @ v[:, 64 * t:64 * t + 64], mn
    return o / l


def test_fault_rescale_skipped_for_one_tile():
    c = SELF("ramp", 257)
    q, k0, v0, _, _ = _split(c)
    assert _worst(c, _join(c, _online(q, k0, v0))) < 1e-6
    for skip in (1, 3, 4):
        _caught(f"no rescale entering tile {skip}", c, _online(q, k0, v0, skip))


def test_fault_v_halves_swapped():
    """the two 32-key halves of a tile swapped for V only"""
    for c, t in ((SELF("diffuse", 64), 0), (SELF("diffuse", 193), 2), (TWO("peaked", 141, 16, 1, 0.7), 1)):
        q, k0, v0, k1, v1 = _split(c)
        vs = v0.clone()
        vs[:, 64 * t:64 * t + 32], vs[:, 64 * t + 32:64 * t + 64] = v0[:, 64 * t + 32:64 * t + 64], v0[:, 64 * t:64 * t + 32]
        w0, w1 = (float(torch.tensor(w, dtype=torch.float32)) for w in c[6:])
        _caught("V halves swapped", c, w0 * _sm(q, k0, vs) + (w1 * _sm(q, k1, v1) if k1 is not None else 0.0))


def test_fault_a_row_takes_the_next_rows_result():
    for c in (("diffuse", B_, H_, 33, 64, 0, 1.0, 0.0), SELF("planted", 129), TWO("ramp", 64, 65, 1, 2)):
        ref = R.ref(*c)[0]
        for i in (0, c[3] - 2):
            out = ref.clone()
            out[:, i] = ref[:, i + 1]
            r = _worst(c, out)
            print(f"[unet-attn] fault `row {i} takes row {i + 1}` at {c}: max(err / bound) {r:.3g}")
            assert r > 1.0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch(lib):
    """every call below is refused on the host: the pointers are never dereferenced and no GPU is needed"""
    INVALID, SHAPE = 1, 2
    p, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    L = lib
    att = lambda Q=p, ldq=64, O=p, ldo=64, nseg=1, K0=p, V0=p, ld0=128, n0=77, K1=None, V1=None, ld1=0, n1=0: L.ia2p_attention(      # noqa: E731
        None, Q, ldq, O, ldo, 1, 1, 128, nseg, K0, V0, ld0, n0, 1.0, K1, V1, ld1, n1, 1.0)
    qp = lambda X=p, W=p, O=p, ldo=64, Nq=128, K=64, nseg=1, K0=p, V0=p, ld0=128, n0=77, K1=None, V1=None, ld1=0, n1=0: L.ia2p_qproj_attention(      # noqa: E731
        None, X, W, None, None, O, ldo, 1, 1, Nq, K, nseg, K0, V0, ld0, n0, 1.0, K1, V1, ld1, n1, 1.0)
    sa = lambda X=p, W=p, O=p, ldo=64, K=192: L.ia2p_qkv_self_attention(None, X, W, None, None, O, ldo, 1, 1, K)      # noqa: E731
    sc = lambda X=p, W=p, O=p, ldo=64, K=192, ctx=p, Lc=81, Li=4, cd=64, Wt=p, Wi=p, kt=p, ki=p, ldkv=128, N=128: L.ia2p_qkv_self_attention_ctx(      # noqa: E731
        None, X, W, None, None, O, ldo, 1, 1, K, ctx, Lc, Li, cd, Wt, Wi, kt, ki, ldkv, N, None)
    cases = [
        (att(Q=None), INVALID), (att(O=None), INVALID), (att(K0=None), INVALID), (att(V0=None), INVALID), (att(nseg=0), INVALID), (att(nseg=3), INVALID),
        (att(nseg=2, K1=None, V1=p, ld1=128, n1=4), INVALID), (att(nseg=2, K1=p, V1=None, ld1=128, n1=4), INVALID),
        (att(n0=0), SHAPE), (att(n0=-1), SHAPE), (att(nseg=2, K1=p, V1=p, ld1=128, n1=0), SHAPE),
        (att(ldq=68), SHAPE), (att(ldo=68), SHAPE), (att(ld0=132), SHAPE), (att(nseg=2, K1=p, V1=p, ld1=132, n1=4), SHAPE), (att(O=odd), SHAPE),
        (qp(X=None), INVALID), (qp(W=None), INVALID), (qp(O=None), INVALID), (qp(K0=None), INVALID), (qp(V0=None), INVALID), (qp(nseg=3), INVALID),
        (qp(nseg=2, K1=p, V1=None, ld1=128, n1=4), INVALID),
        (qp(Nq=200), SHAPE), (qp(Nq=0), SHAPE), (qp(K=100), SHAPE), (qp(K=0), SHAPE), (qp(n0=0), SHAPE), (qp(nseg=2, K1=p, V1=p, ld1=128, n1=0), SHAPE),
        (qp(ldo=68), SHAPE), (qp(ld0=132), SHAPE), (qp(nseg=2, K1=p, V1=p, ld1=132, n1=4), SHAPE), (qp(O=odd), SHAPE),
        (sa(X=None), INVALID), (sa(W=None), INVALID), (sa(O=None), INVALID), (sa(K=100), SHAPE), (sa(K=0), SHAPE), (sa(ldo=68), SHAPE), (sa(O=odd), SHAPE),
        (sc(X=None), INVALID), (sc(O=None), INVALID), (sc(ctx=None), INVALID), (sc(Wt=None), INVALID), (sc(kt=None), INVALID), (sc(Wi=None), INVALID), (sc(ki=None), INVALID),
        (sc(K=100), SHAPE), (sc(ldo=68), SHAPE), (sc(O=odd), SHAPE), (sc(Li=81), SHAPE), (sc(Li=-1), SHAPE), (sc(cd=100), SHAPE), (sc(N=100), SHAPE), (sc(ldkv=120), SHAPE),
        (sc(ldkv=132), SHAPE), (sc(kt=odd), SHAPE), (sc(ki=odd), SHAPE),
    ]
    for i, (got, want) in enumerate(cases):
        assert got == want, f"case {i}: status {got}, expected {want}"
