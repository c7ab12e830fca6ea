"""fp64 reference of the UNet's fused attention -- `ia2p_attention`, and through it the attention halves of `ia2p_qproj_attention` and `ia2p_qkv_self_attention`
(csrc/attention.hip, csrc/attention_core.h, the two fused launches of csrc/qxattn.hip) -- and the element-wise error bound its kernel must meet. Written in the manner
of attn_ops_ref.py, whose `_core` it drives with a kind of its own (`unet`) and whose notation it keeps: u = 2^-24, SECOND covers second-order terms.

    out = w0 softmax(Q K0^T / 8) V0 [+ w1 softmax(Q K1^T / 8) V1]          two independent softmaxes, head dimension 64

computed in float64 from exactly the fp16 bits the kernel is given, w0 and w1 as the fp32 numbers the entry point receives. `unet_attention` returns
(ref, bound, (exp_share, mfma_share)). Every term of the bound is read off attention_core.h, none off what a kernel returned. With natural-log scores s_j = q . k_j / 8,
x_j = s_j - max s, e_j = exp(x_j), S = sum e, w_j = e_j / S, a score error d_j moves a softmax output by at most sum_j w_j |d_j| |v_j - out| (attn_ops_ref.py (*): what
is common to all keys of a row cancels). Per segment, d_j is the sum of

  score          S^T = K . Q^T: 64 exact fp16 x fp16 products accumulated in fp32 by four v_mfma_f32_32x32x16_f16. How an addition inside an fp16 MFMA rounds is not
                 documented: MODELLED as the 16x16x16 one is, each addition off by at most one fp32 ulp (2 u) in any order, 2 D u sum |q k| / 8 with D the products
                 that are not 0 (`_nnz`).
  exponent       p = exp2(st c - fl(m_t c)) on the RAW accumulator st, c = scale_log2e = 0.125f * 1.4426950408889634f (log2 e rounded to fp32, the product with 1 / 8
                 exact: u), m_t the running maximum up to and including the key's 64-key tile. Packed form (IA2P_ATTN_PK): fl(fl(st c) - fl(m_t c)), three roundings,
                 u (|s_j| + |m_t| + |s_j - m_t|) in natural units; fused by the compiler (or the fmaf of the image-token tile): u (|m_t| + |s_j - m_t|). The error of
                 c itself: u |s_j - m_t|. The bound takes the larger sum, so it holds either way: u (|s_j| + |m_t| + 2 |x_j|)  (|s_j - m_t| <= |x_j|).
                 u |m_t| is common to the keys of ONE tile only: it does not cancel across tiles, see the rescale.
  exponential    v_exp_f32, MODELLED as in encoder_ops_ref: X_j = (|x_j| + 4) 2^-23.
  rescale        when the running maximum rises, o and lrun are multiplied by alpha = exp2(fl(fl(m_old - m_new) c)). A consistent kernel would use
                 exp2(fl(m_old c) - fl(m_new c)); it does not, so what remains of key j's exponent after all later alphas is s_j c - m c + (fl(m_t c) - m_t c) + the
                 roundings of the alpha exponents: the u |m_t| above (already counted, per tile), and per later rise the subtraction, the product and c's error,
                 3 u |dm|, which telescope into 3 u (m - m_t). Each alpha is a native exponential: (|dm| + 4) 2^-23 under the model; the |dm| parts are inside |x_j|,
                 4 2^-23 per later tile with a rising maximum is added to X_j. One rounding of the product per tile on o and on lrun: nl u (sum w |v| + |out|).
On the numerator alone:
  fp16 p         every p_j is rounded to fp16 (v_cvt_pk_f16_f32, subnormals kept) before P.V while lrun adds the unrounded p_j: half an fp16 ulp of p_j taken against
                 m_t (2^-25 absolute below the normal range, p_j itself where it rounds to 0), scaled down by the later alphas. THIS TERM AND THE fp16 STORE DECIDE
                 ALMOST EVERY CASE; a planted row has p = 1 exactly and is decided by the store alone.
  P.V            O^T += V^T . P^T in 16-key v_mfma_f32_32x32x16_f16, in program order on one accumulator per 32 output channels; each MODELLED as 16 additions off by
                 2 u in any order: 2 u cnt_j w_j |v_j|, cnt_j the keys with a non-zero fp16 p of key j's MFMA and of every later one (adding 0 is exact).
On the denominator alone: the sum of nkeys positive terms in any order (two packed lanes, two lane halves, the shuffle), (nkeys + 2) u; then w = fl(w0 / l) and the
product o w: (nkeys + 5) u |out| covers them.

MODE 0 (one segment) is exactly that, times w0.

MODE 1 (a second segment of <= 64 image-token keys, w0 != 0: one merged accumulator). The text segment runs as above but is not divided yet; l_text is final after
its last tile. The image-token tile has its own maximum and its own sum l_ip (fmaf exponent: covered by the exponent term; (n1 + 2) u for the sum); its
probabilities are multiplied by ci = fl(fl(fl(w1 / w0) l_text) / l_ip) (3 u), the product rounded (u) and then rounded to fp16: HALF AN fp16 ULP OF e_i ci, 2^-25
absolute in the subnormal range and e_i ci itself where it rounds to 0 -- ci can be far from 1 (l_text up to n0, l_ip >= 1), so this is not the half ulp of a
probability. The common final factor fl(w0 / l_text) (u) and its product (u) bring the image part to w1 / l_ip sum e_i v_i: the computed l_text is the SAME fp32 number
in ci and in the final factor and cancels, so the image part carries (n1 + 8) u |w1 out_ip| and, in absolute terms, (|w0| / l_text) sum_i half_ulp(e_i ci) |v_i|.
The P.V chain goes on through the image-token MFMAs: a text key's cnt_j grows by the image-token keys whose fp16 p is not 0 (`tail`).
  folded form    (attn_fold_ok: n0 % 64 != 0, n1 <= 32, n0 % 64 + n1 <= 64) the image-token keys sit in the free slots of the last text tile. The two softmaxes take
                 the same numbers -- a key-index mask keeps them apart -- and ci is formed from the same l_text; what differs is the order of the sums (any order is
                 what the bound assumes) and the P.V chain: an image-token key shares its 16-key MFMA with up to 15 text keys, so its cnt_i is the image-token keys
                 + 15 in every fold-eligible case, folded or not. One bound serves both forms.

MODE 2 (any other two-segment call; w0 = 0 selects it): each segment as MODE 0 with its own accumulator, scaled by fl(w_s / l_s) in fp32 and summed into otot:
|w0| B_0 + |w1| B_1 + u |out| for the one addition that is not an addition to 0.

Store           the fp16 store of the sum: half an ulp at |out| + B (`with_store16`).

The two MODELS (the native exponential, the 2 u per MFMA addition) cannot be verified without the hardware: every case keeps each model's share of its bound at or
below a tenth (`_check_shares`; test_unet_attn_cpu.py asserts it for every GPU case). V = 1 + randn / 4 everywhere, so no output cancels; the families whose scores are
large by construction (peaked, ramp, planted) use queries with few non-zero channels, which costs the score model nothing where the products are exactly 0.
"""
import functools

import numpy as np
import torch

from attn_ops_ref import A_K, B_Q, _check_shares, _core, _nnz, _onehot, _rn, _v, gen  # noqa: F401
from encoder_ops_ref import _exp_model, with_store16  # noqa: F401
from llm_ops_ref import SECOND, U, f64, half_ulp16, ratio  # noqa: F401

DH = 64
FAMILIES = ("diffuse", "peaked", "ramp", "planted")


def fold_ok(n0, n1):
    """attn_fold_ok of attention_core.h"""
    return n0 % 64 != 0 and 0 < n1 <= 32 and n0 % 64 + n1 <= 64


def mode(n1, w0):
    """the kernel template ia2p_launch_attention picks"""
    return 0 if not n1 else (1 if n1 <= 64 and float(np.float32(w0)) != 0.0 else 2)


def _heads(t, heads):
    """fp16 [B, n, heads 64] -> fp64 [B heads, n, 64]"""
    B, n, _ = t.shape
    return f64(t).reshape(B, n, heads, DH).transpose(1, 2).reshape(B * heads, n, DH)


def _scores(q, k):
    s = (q @ k.transpose(1, 2)) * 0.125
    return s, U * s.abs(), 2 * U * 0.125 * _nnz(q, k) * (q.abs() @ k.abs().transpose(1, 2))


def _lin(w, delta, v, out):
    """sum_j w_j delta_j |v_j - out|, term by term (the image-token tile: at most 64 keys)"""
    return ((w * delta).unsqueeze(-1) * (v.unsqueeze(1) - out.unsqueeze(2)).abs()).sum(2)


def _ip_tile(q, k1, v1, w0, w1, Lt, folds):
    """the image-token tile of MODE 1 -> (out_ip, plain, model, ex, tail): absolute errors of w1 out_ip, and the keys whose fp16 p is not 0"""
    n1 = k1.shape[1]
    s, Dn, Dm = _scores(q, k1)
    m = s.max(-1, keepdim=True).values
    x = s - m
    e = torch.exp(x)
    L = e.sum(-1, keepdim=True)
    w = e / L
    out = w @ v1
    va = v1.abs()
    pc = e * (abs(w1) / abs(w0)) * Lt / L * 1.001
    nz = (pc >= 2.0 ** -25).double()
    nt = -(-n1 // 16)
    per = torch.nn.functional.pad(nz, (0, nt * 16 - n1)).reshape(*s.shape[:-1], nt, 16).sum(-1)
    cnt = per.flip(-1).cumsum(-1).flip(-1).repeat_interleave(16, -1)[..., :n1] + (15 if folds else 0)
    h = torch.minimum(pc, half_ulp16(pc))
    plain = abs(w1) * (_lin(w, Dn + U * (m.abs() + 2 * x.abs()), v1, out) + (n1 + 8) * U * out.abs()) + (abs(w0) / Lt) * (h @ va)
    model = abs(w1) * (_lin(w, Dm, v1, out) + 2 * U * ((w * cnt) @ va))
    ex = abs(w1) * _lin(w, _exp_model(x), v1, out)
    return out, plain, model, ex, nz.sum(-1, keepdim=True)


def unet_attention(q, k0, v0, k1, v1, w0, w1, heads):
    """q fp16 [B, Nq, heads 64], k0 / v0 [B, n0, heads 64], k1 / v1 [B, n1, heads 64] or None -> (out [B, Nq, heads 64], bound, shares)"""
    B, Nq, _ = q.shape
    w0, w1 = float(np.float32(w0)), float(np.float32(w1))
    n0, n1 = k0.shape[1], 0 if k1 is None else k1.shape[1]
    md = mode(n1, w0)
    qq, K0, V0 = _heads(q, heads), _heads(k0, heads), _heads(v0, heads)
    s0, Dn0, Dm0 = _scores(qq, K0)
    if md == 0:
        o, plain, model, ex, _ = _core(s0, Dn0, Dm0, V0, "unet", parts=True)
        out, plain, model, ex = w0 * o, abs(w0) * plain, abs(w0) * model, abs(w0) * ex
    else:
        K1, V1 = _heads(k1, heads), _heads(v1, heads)
        if md == 1:
            Lt = torch.exp(s0 - s0.max(-1, keepdim=True).values).sum(-1, keepdim=True)
            o1, p1, m1, e1, tail = _ip_tile(qq, K1, V1, w0, w1, Lt, fold_ok(n0, n1))
            o0, p0, m0, e0, S = _core(s0, Dn0, Dm0, V0, "unet", tail=tail, parts=True)
            assert torch.allclose(S, Lt, rtol=1e-12, atol=0.0)
            out, plain = w0 * o0 + w1 * o1, abs(w0) * p0 + p1
            model, ex = abs(w0) * m0 + m1, abs(w0) * e0 + e1
        else:
            s1, Dn1, Dm1 = _scores(qq, K1)
            o0, p0, m0, e0, _ = _core(s0, Dn0, Dm0, V0, "unet", parts=True)
            o1, p1, m1, e1, _ = _core(s1, Dn1, Dm1, V1, "unet", parts=True)
            out = w0 * o0 + w1 * o1
            plain = abs(w0) * p0 + abs(w1) * p1 + U * out.abs()
            model, ex = abs(w0) * m0 + abs(w1) * m1, abs(w0) * e0 + abs(w1) * e1
    bound = with_store16(out, SECOND * (plain + model + ex))
    shares = (float((SECOND * ex / bound).max()), float((SECOND * model / bound).max()))
    fold = lambda t: t.reshape(B, heads, Nq, DH).transpose(1, 2).reshape(B, Nq, heads * DH)      # noqa: E731
    return fold(out), fold(bound), _check_shares(shares, f"unet_attention Nq={Nq} n0={n0} n1={n1} w=({w0}, {w1})")


# ---- the cases of the GPU tests (built on the CPU; test_unet_attn_cpu.py checks the two shares for every one) -----------------------------------------------------
# The sizes are the smallest that reach each branch of the kernel, not the workload's. B = 2 and 3 heads: 6, 12, 18 or 30 workgroups, no multiple of 8
# (but at 385 tokens: four query blocks at B = 2 are 8 heads workgroups whatever the heads).
B_, HEADS = 2, 3
SELF_N = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 385, 513)      # Nq = nkeys, packed qkv: every DMA stage edge (128 keys, two buffers)
CROSS = ((1, 77), (31, 77), (33, 64), (127, 129), (129, 13), (160, 96), (257, 77), (384, 192))       # (Nq, nkeys)
CROSS_ONE_WG = (1, 1, 33, 77)                  # (B, heads, Nq, nkeys): a single workgroup
CROSS_NINE_WG = (1, 3, 300, 77)                # three query blocks x three heads: nwg = 9
TWO_NQ = 160                                   # two query blocks, the second a quarter full
FOLDED = ((77, 4, 1, 1), (77, 4, 0.5, 1.3), (13, 4, 2, 0.9), (63, 1, 1, 1), (31, 1, 1, 0.7), (28, 4, 1, 1), (29, 4, 1, 1), (32, 32, 1, 1), (96, 32, 0.75, 1), (141, 16, 1, 0.7),
          (77, 4, 1, 0))                       # (Lt, Li, w0, w1): MODE 1, resident, attn_fold_ok
NOT_FOLDED = ((64, 4, 1, 1), (33, 32, 1, 1), (77, 33, 1, 1), (192, 64, 1, 1.3), (128, 16, 0.5, 0.7))      # MODE 1, resident
STREAMED = ((257, 4, 1, 0.9), (256, 64, 2, 1), (300, 4, 1, 0.9))                                          # MODE 1, more than four key tiles
MODE2 = ((64, 65, 1, 2), (77, 100, 1, 0.5), (300, 100, 0.5, 0.5), (77, 4, 0, 1))                          # (a zero first weight selects MODE 2)
TWO = FOLDED + NOT_FOLDED + STREAMED + MODE2
LAYOUT_PADS = (8, 64)                          # ldo = heads 64 + pad
LAYOUT_ONE = ((2, 3, 33, 33), (2, 3, 129, 13), (2, 3, 257, 77))      # (B, heads, Nq, nkeys): clamped rows q >= Nq in the last query block of each
LAYOUT_TWO = ((77, 4, 0.5, 1.3), (64, 65, 1, 2))
QPROJ_ONE = (13, 32, 33, 77, 96, 160, 192)     # one segment through the fused launch: nkh == 1 and the PRE staging in MODE 0
QPROJ_NQ = (128, 384)
SATTN_N = 256
# Input adjustment for the share cap. peaked at 513 keys (SELF_N's largest): with the weight on a few keys anywhere in the key order, the any-order P.V model of the
# 33 MFMAs behind an early key is 0.103 of the bound. Above PEAKED_LATE keys the peaked scores also rise by 8 along the key order (channel 0, as the ramp family): the
# keys that carry a row sit late in the chain, cnt_j is small where w_j is not. The shape and the family stay.
PEAKED_LATE = 384


def resident3(n0, n1):
    """attn_kv_resident: at most three key tiles, what the fused to_q launch takes"""
    return -(-n0 // 64) + -(-n1 // 64) <= 3


QPROJ_TWO = tuple(c for c in TWO if resident3(c[0], c[1]))
QPROJ_384 = ((77, 0, 1, 0), (192, 0, 1, 0), (77, 4, 0.5, 1.3), (64, 65, 1, 2))      # the cases repeated at three query blocks per (image, head)


def edges(n, second=False):
    """the planted keys of a segment: 0, 31, 32, 63, 64, 127 / 128 (the DMA stage edge) and the last live key; the first and the last image-token key"""
    return sorted({e for e in ((0, n - 1) if second else (0, 31, 32, 63, 64, 127, 128, n - 1)) if e < n})


def ramp_rise(n):
    """how far the natural-log scores of the ramp family rise over a segment of n keys: 1.5 per 64-key tile, 3 at least"""
    return max(3.0, 1.5 * n / 64)


@functools.lru_cache(maxsize=None)
def case(family, B, heads, Nq, n0, n1=0, w0=1.0, w1=0.0):
    """-> (q [B, Nq, heads 64], k0, v0 [B, n0, heads 64], k1, v1 [B, n1, heads 64] or None, want) in fp16, from a seed fixed by the arguments. Families:
    diffuse  q, k ~ N(0, 1): scores ~ N(0, 1)
    peaked   q ~ N(0, 3^2) on 16 channels (0 elsewhere), k ~ N(0, 2^2): scores ~ N(0, 3^2), a few keys carry each row
    ramp     q is 4 on channel 0, N(0, 0.5^2) on channels 1 .. 7 and 0 elsewhere; k ~ N(0, 0.5^2) with channel 0 rising linearly along the key order: the scores rise
             by ramp_rise(n) over the segment on a noise of 0.1, the running maximum rises in every tile and alpha != 1 throughout
    planted  query i leads by 28 or more on key edges0[i % len] of segment 0 (and, independently, on key edges1[(i // len) % len1] of segment 1, through channels
             32 ..): want = w0 v_a [+ w1 v_b] from the fp16 value rows, which with one segment of weight 1 the output must equal to the bit
    V = 1 + randn / 4 throughout."""
    g = gen(((FAMILIES.index(family) * 1009 + Nq) * 1013 + n0) * 1019 + 7 * n1 + 3 * heads + B)
    segs = [n0] + ([n1] if n1 else [])
    q = _rn(g, B, Nq, heads, DH)
    ks, vs = [_rn(g, B, n, heads, DH) for n in segs], [_v(g, B, n, heads, DH) for n in segs]
    want = None
    if family == "peaked":
        q[..., 16:] = 0.0
        q, ks = 3.0 * q, [2.0 * k for k in ks]
        if n0 > PEAKED_LATE:      # (385 and 513 keys) the share cap, see PEAKED_LATE
            q[..., 0] = 4.0
            ks[0][..., 0] = (16.0 * torch.arange(n0).double() / n0).reshape(1, n0, 1)
    elif family == "ramp":
        q[..., 8:] = 0.0
        q = 0.5 * q
        q[..., 0] = 4.0
        ks = [0.5 * k for k in ks]
        for k, n in zip(ks, segs):
            k[..., 0] = (2.0 * ramp_rise(n) * torch.arange(n).double() / n).reshape(1, n, 1)
    elif family == "planted":
        i = torch.arange(Nq)
        e0 = edges(n0)
        slots = [i % len(e0)] + ([(i // len(e0)) % len(edges(n1, True))] if n1 else [])
        q = sum(_onehot(sl + 32 * j, DH, B_Q) for j, sl in enumerate(slots)).reshape(1, Nq, 1, DH).expand(B, Nq, heads, DH)
        ks = [0.05 * k for k in ks]
        want = 0.0
        for j, (k, v, n, sl, w) in enumerate(zip(ks, vs, segs, slots, (w0, w1))):
            ed = edges(n, bool(j))
            for a, e in enumerate(ed):
                k[:, e] = _onehot(torch.tensor(a + 32 * j), DH, A_K)
            want = want + float(np.float32(w)) * v.half().double()[:, torch.tensor(ed)[sl]]
        want = want.reshape(B, Nq, heads * DH)
    h = lambda t: t.reshape(B, -1, heads * DH).half().contiguous()      # noqa: E731
    return (h(q), h(ks[0]), h(vs[0])) + ((h(ks[1]), h(vs[1])) if n1 else (None, None)) + (want,)


@functools.lru_cache(maxsize=None)
def ref(family, B, heads, Nq, n0, n1=0, w0=1.0, w1=0.0):
    q, k0, v0, k1, v1, _ = case(family, B, heads, Nq, n0, n1, w0, w1)
    return unet_attention(q, k0, v0, k1, v1, w0, w1, heads)


def shapes():
    """every (B, heads, Nq, n0, n1, w0, w1) the GPU tests launch, once"""
    out = [(B_, HEADS, n, n, 0, 1.0, 0.0) for n in SELF_N]
    out += [(B_, HEADS, nq, nk, 0, 1.0, 0.0) for nq, nk in CROSS]
    out += [CROSS_ONE_WG + (0, 1.0, 0.0), CROSS_NINE_WG + (0, 1.0, 0.0)]
    out += [(B_, HEADS, TWO_NQ, lt, li, float(a), float(b)) for lt, li, a, b in TWO]
    out += [s + (0, 1.0, 0.0) for s in LAYOUT_ONE]
    out += [(B_, HEADS, QPROJ_NQ[0], n, 0, 1.0, 0.0) for n in QPROJ_ONE]
    out += [(B_, HEADS, QPROJ_NQ[0], lt, li, float(a), float(b)) for lt, li, a, b in QPROJ_TWO]
    out += [(B_, HEADS, QPROJ_NQ[1], lt, li, float(a), float(b)) for lt, li, a, b in QPROJ_384]
    return list(dict.fromkeys(out))


def all_cases():
    for shape in shapes():
        for family in FAMILIES:
            yield (family,) + shape
