"""fp64 reference of the regional IP-Adapter cross-attention -- `ia2p_attention_regions` (csrc/attention_regions.hip) -- and of the mask pyramid `ia2p_region_levels`, and
the element-wise error bound the attention kernel must meet. Written in the manner of unet_attn_ref.py, whose helpers and notation it imports: u = 2^-24, SECOND covers
second-order terms, s_j = q . k_j / 8 the natural-log scores.

    out[b, q, h, :] = w0 softmax_j(q . k_text_j / 8) v_text_j + sum_{g < G} s[b] m[b, g, q] softmax_{j in group g}(q . k_ip_j / 8) v_ip_j

computed in float64 from exactly the fp16 bits the kernel is given (Q, K, V and the mask weights m), w0 and s[b] as the fp32 numbers the entry point receives.
`region_attention` returns (ref, bound, (exp_share, mfma_share)). Every term is read off attention_regions.hip, none off what a kernel returned.

The text segment is the text segment of MODE 1 of unet_attn_ref.py, instruction for instruction (packed exponent, online maximum, alpha rescale, fp16 p, one merged
accumulator divided by l_text at the very end): `_core(..., "unet", tail=...)` times |w0|, `tail` the image-token keys whose fp16 probability is not 0 -- THE LONGER
P.V CHAIN: up to 64 keys in four more 16-key MFMAs behind every text key (MODE 1 as launched by the UNet has 4).

The image-token tile: group g is keys 4 g .. 4 g + 3, four accumulator registers of one lane. Per group
  score, exponent, exponential   as the image-token tile of MODE 1 (`_ip_tile`): the modelled MFMA score 2 D u sum |q k| / 8, u |s_j| for c = scale_log2e, the fmaf
                 exponent u (|m_g| + 2 |x_j|) against the GROUP's own maximum m_g, v_exp_f32 modelled (|x_j| + 4) 2^-23; through (*) of attn_ops_ref.py per group:
                 sum_{j in g} w_j d_j |v_j - out_g|, times |s[b] m|.
  m              fp16 in device memory, converted to fp32 exactly: THE ROUNDING OF m happens on the host or in the pyramid, before the launch; the reference takes the
                 same fp16 bits, so the launch adds nothing for it. (The pyramid's one rounding is checked to the bit on its own.)
  coefficient    c_g = fl(fl(fl(fl(s[b] / w0) m) l_text) / l_g): FOUR roundings, 4 u -- the chain s[b] m / w0 l_text / l_g with the division by w0 hoisted out of the
                 groups. l_g = ((e_0 + e_1) + e_2) + e_3: three additions of positive terms, 3 u (counted as 4 + 2 the way MODE 1 counts n1 + 2). The product e_j c_g
                 (u); the final factor fl(w0 / l_text) and its product (2 u). The computed l_text is the SAME fp32 number in c_g and in the final factor and cancels.
                 Together (4 + 2) + 4 + 1 + 2 = 13 u |s[b] m out_g|.
  fp16 p         e_j c_g is rounded to fp16 before P.V: HALF AN fp16 ULP OF e_j c_g (2^-25 absolute in the subnormal range, e_j c_g itself where it rounds to 0), as
                 the MODE 1 text explains -- c_g = s m l_text / (w0 l_g) is far from 1 when l_text is. In absolute terms (|w0| / l_text) sum_j half_ulp(e_j |c_g|) |v_j|.
                 m == 0 (or a padded group) selects c_g = +0 exactly: p = +0, no error and no MFMA addition that is not an addition of 0.
  P.V            the tile's four (4 G <= 32: two) 16-key MFMAs go on in the text accumulator: 2 u cnt_j |s m| w_j |v_j|, cnt_j the image-token keys with a non-zero fp16
                 p in key j's MFMA and the later ones.
Store            half an fp16 ulp at |out| + B (`with_store16`).

No folded form exists: the image-token keys always sit in a tile of their own, so one bound serves.

With one group and m == 1 the formula is the two-segment formula of unet_attn_ref.unet_attention at n1 = 4, w1 = s, and with every m == 0 its one-segment formula; the GPU
test holds the launch to THOSE bounds there. The two MODELS (native exponential, 2 u per MFMA addition) keep at most a tenth of the bound in every case
(`_check_shares`; test_region_attn_cpu.py asserts it for every GPU case).

The pyramid. out[b, g, y, x] = mean of the f x f block, summed in fp32 in row-major order, scaled by the exact 1 / f^2 and rounded once to fp16. The fp32 sum of f^2
fp16 numbers is exact when they are multiples of 2^-k with f^2 max|m| 2^k < 2^24 -- the masks of `levels_case` are multiples of 2^-10 in [0, 1.5], {0, 1} masks
included -- so the result is the float64 mean rounded to fp16 once (`levels`), to the bit.
"""
import functools

import numpy as np
import torch

import unet_attn_ref as UA
from unet_attn_ref import DH, FAMILIES, SECOND, U, _check_shares, _core, _exp_model, _heads, _scores, f64, half_ulp16, ratio, with_store16  # noqa: F401
from encoder_ops_ref import round16  # noqa: F401

TOK = 4                                        # image tokens per group (ImageProjModel's num_tokens)
MASKS = ("rect", "ramp", "zero", "one", "big")


def region_attention(q, k0, v0, k1, v1, w0, s, m, heads):
    """q fp16 [B, Nq, heads 64], k0 / v0 [B, n0, heads 64], k1 / v1 [B, 4 G, heads 64], s: B floats, m fp16 [B, G, Nq] -> (out [B, Nq, heads 64], bound, shares)"""
    B, Nq, _ = q.shape
    G = m.shape[1]
    n0 = k0.shape[1]
    assert k1.shape[1] == TOK * G and m.shape == (B, G, Nq)
    w0 = float(np.float32(w0))
    sb = torch.tensor([float(np.float32(x)) for x in s], dtype=torch.float64)
    qq, K0, V0, K1, V1 = (_heads(t, heads) for t in (q, k0, v0, k1, v1))
    BH = B * heads
    coef = (sb.reshape(B, 1, 1) * f64(m)).transpose(1, 2)                                # [B, Nq, G]
    coef = coef.unsqueeze(1).expand(B, heads, Nq, G).reshape(BH, Nq, G)
    # text
    s0, Dn0, Dm0 = _scores(qq, K0)
    Lt = torch.exp(s0 - s0.max(-1, keepdim=True).values).sum(-1, keepdim=True)
    # image-token groups: everything [BH, Nq, G, 4]
    s1, Dn1, Dm1 = (t.reshape(BH, Nq, G, TOK) for t in _scores(qq, K1))
    mg = s1.max(-1, keepdim=True).values
    x = s1 - mg
    e = torch.exp(x)
    Lg = e.sum(-1, keepdim=True)
    w = e / Lg
    Vg = V1.reshape(BH, 1, G, TOK, DH)
    og = (w.unsqueeze(-1) * Vg).sum(3)                                                   # [BH, Nq, G, 64]
    ca = coef.abs().unsqueeze(-1)                                                        # [BH, Nq, G, 1]
    dev = (Vg - og.unsqueeze(3)).abs()                                                   # [BH, Nq, G, 4, 64]
    va = Vg.abs()
    lin = lambda d: ((ca * w * d).unsqueeze(-1) * dev).sum((2, 3))                       # noqa: E731  (*) per group, summed over the groups
    pc = e * ca / abs(w0) * Lt.unsqueeze(-1) / Lg * 1.001
    nz = (pc >= 2.0 ** -25).double().reshape(BH, Nq, G * TOK)
    nt = -(-(G * TOK) // 16)
    per = torch.nn.functional.pad(nz, (0, nt * 16 - G * TOK)).reshape(BH, Nq, nt, 16).sum(-1)
    cnt = per.flip(-1).cumsum(-1).flip(-1).repeat_interleave(16, -1)[..., :G * TOK].reshape(BH, Nq, G, TOK)
    h = torch.minimum(pc, half_ulp16(pc))
    out_ip = (coef.unsqueeze(-1) * og).sum(2)
    plain_ip = lin(Dn1 + U * (mg.abs() + 2 * x.abs())) + 13 * U * (ca * og.abs()).sum(2) + (abs(w0) / Lt) * (h.unsqueeze(-1) * va).sum((2, 3))
    model_ip = lin(Dm1) + 2 * U * ((ca * w * cnt).unsqueeze(-1) * va).sum((2, 3))
    ex_ip = lin(_exp_model(x))
    tail = nz.sum(-1, keepdim=True)
    o0, p0, m0, e0, S = _core(s0, Dn0, Dm0, V0, "unet", tail=tail, parts=True)
    assert torch.allclose(S, Lt, rtol=1e-12, atol=0.0)
    out = w0 * o0 + out_ip
    plain, model, ex = abs(w0) * p0 + plain_ip, abs(w0) * m0 + model_ip, abs(w0) * e0 + ex_ip
    bound = with_store16(out, SECOND * (plain + model + ex))
    shares = (float((SECOND * ex / bound).max()), float((SECOND * model / bound).max()))
    fold = lambda t: t.reshape(B, heads, Nq, DH).transpose(1, 2).reshape(B, Nq, heads * DH)      # noqa: E731
    return fold(out), fold(bound), _check_shares(shares, f"region_attention Nq={Nq} n0={n0} G={G} w0={w0}")


# ---- the mask weights ----------------------------------------------------------------------------------------------------------------------------------------------
GRIDS = {16: (4, 4), 64: (8, 8), 160: (10, 16), 256: (16, 16), 128: (8, 16)}      # Nq -> the (h, w) the query index runs over, row-major


@functools.lru_cache(maxsize=None)
def masks(kind, B, G, Nq):
    """fp16 [B, G, Nq], the two rows different. Kinds:
    rect   disjoint {0, 1} rectangles: group g owns a band of columns in row 0 of the batch, a band of rows in row 1 (a grid with fewer bands than groups leaves groups empty)
    ramp   soft overlapping ramps along the query order, peak 1 at the group's centre, neighbours overlap; row 1 runs the other way
    zero   ramp with one group all zero        one    ramp with one group all one        big    ramp times 1.5"""
    h, w = GRIDS[Nq]
    yy, xx = torch.arange(Nq) // w, torch.arange(Nq) % w
    g = torch.arange(G).reshape(G, 1)
    if kind == "rect":
        m = torch.stack([(xx * G // w).reshape(1, Nq) == g, (yy * G // h).reshape(1, Nq) == g]).double()
    else:
        t = (torch.arange(Nq).double() + 0.5) / Nq
        c = (g.double() + 0.5) / G
        r0 = (1 - (t.reshape(1, Nq) - c).abs() * G / 1.5).clamp(0, 1)
        m = torch.stack([r0, r0.flip(-1)])
        if kind == "zero":
            m[:, G // 2] = 0.0
        elif kind == "one":
            m[:, G // 2] = 1.0
        elif kind == "big":
            m = 1.5 * m
    if B != 2:
        m = m[:1].expand(B, G, Nq) if B == 1 else torch.cat([m] * (-(-B // 2)))[:B]
    return m.half().contiguous()


# ---- the cases of the GPU test (built on the CPU; test_region_attn_cpu.py checks the two shares for every one) ------------------------------------------------------
# (B, heads, Nq, n0, G, mask kind, w0). B = 2 throughout: the two rows carry different masks and different s[b] (S_B). The sizes are the smallest that reach each branch:
#   Nq   16 (less than one wave's 32 rows), 64, 160 (a full workgroup plus a clamped tail), 256
#   n0   77 (partial last text tile), 64 (no partial tile), 120 (a last tile with room for two groups, were they folded, but not three), 300 (five text tiles: the
#        streamed staging, the image-token tile staged on its own)
#   G    1, 2, 3, 8 (one half of the tile, full), 9 (36 keys: the second half, past one staging chunk), 16 (the full 64-key tile)
S_B = (0.8, 0.5)
NQ_SWEEP = ((2, 2, 16, 77, 3, "rect", 1.0), (2, 5, 64, 77, 3, "ramp", 1.0), (2, 2, 160, 77, 3, "zero", 1.0), (2, 2, 256, 77, 3, "one", 1.0))
G_SWEEP = ((2, 2, 160, 77, 1, "big", 1.0), (2, 5, 160, 77, 2, "rect", 1.0), (2, 2, 160, 77, 8, "ramp", 1.0), (2, 2, 160, 77, 9, "zero", 1.0), (2, 2, 160, 77, 16, "big", 1.0))
N0_SWEEP = ((2, 2, 160, 64, 3, "one", 0.75), (2, 2, 160, 120, 3, "ramp", 1.0), (2, 2, 160, 300, 3, "rect", 1.0))
MASK_SWEEP = ((2, 2, 160, 77, 3, "rect", 1.0), (2, 2, 160, 77, 3, "ramp", 1.0), (2, 2, 160, 77, 3, "one", 1.0), (2, 2, 160, 77, 3, "big", 0.5))      # "zero" is in NQ_SWEEP
SHAPES = tuple(dict.fromkeys(NQ_SWEEP + G_SWEEP + N0_SWEEP + MASK_SWEEP))
BASE = (2, 2, 160, 77, 3)                      # the shape of the property tests (locality, padding)


@functools.lru_cache(maxsize=None)
def case(family, B, heads, Nq, n0, G, kind, w0):
    """-> (q, k0, v0, k1, v1, m): Q / K / V of unet_attn_ref.case (family: diffuse, peaked, ramp, planted) with a second segment of 4 G keys, the masks of `masks`"""
    q, k0, v0, k1, v1, _ = UA.case(family, B, heads, Nq, n0, TOK * G, w0, 1.0)
    return q, k0, v0, k1, v1, masks(kind, B, G, Nq)


@functools.lru_cache(maxsize=None)
def ref(family, B, heads, Nq, n0, G, kind, w0):
    q, k0, v0, k1, v1, m = case(family, B, heads, Nq, n0, G, kind, w0)
    return region_attention(q, k0, v0, k1, v1, w0, S_B[:B], m, heads)


def all_cases():
    for shape in SHAPES:
        for family in FAMILIES:
            yield (family,) + shape


# ---- ia2p_region_levels --------------------------------------------------------------------------------------------------------------------------------------------
LEVEL_F, LEVEL_HW, LEVEL_B, LEVEL_G = (1, 2, 4), ((16, 16), (12, 20)), 2, 3


def levels(m, f):
    """m fp16 [B, G, h, w] -> fp64 [B, G, (h / f) (w / f)]: the float64 mean of each f x f block, rounded to fp16 once"""
    B, G, h, w = m.shape
    return round16(f64(m).reshape(B, G, h // f, f, w // f, f).mean((3, 5)).reshape(B, G, -1))


@functools.lru_cache(maxsize=None)
def levels_case(kind, h, w):
    """fp16 [LEVEL_B, LEVEL_G, h, w]: `binary` {0, 1}; `soft` multiples of 2^-10 in [0, 1.5] (docstring: the fp32 sum is exact)"""
    g = UA.gen(7 * h + w + len(kind))
    r = torch.rand(LEVEL_B, LEVEL_G, h, w, generator=g, dtype=torch.float64)
    return ((r < 0.5).double() if kind == "binary" else torch.round(1.5 * r * 1024) / 1024).half()
