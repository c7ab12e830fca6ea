"""fp64 references of the three attention launches that are not causal -- `ia2p_attention_full` (csrc/vit.hip), `ia2p_attention_window_relpos` /
`ia2p_attention_global_relpos` and `ia2p_attention_small_head` (csrc/sam.hip) -- and of `ia2p_mask_upsample_threshold` and `ia2p_mask_morph`, and next to each the
error bound its HIP kernel must meet. Written in the manner of encoder_ops_ref.py and llm_ops_ref.py, whose notation and helpers it imports: u = 2^-24, SECOND
covers second-order terms.

Every reference takes exactly the bits the kernel is given and computes in float64; every bound is derived from the operations in the kernel source, none from
what a kernel returned. The attention references return (ref, bound, (exp_share, mfma_share)).

The attention bound. With natural-log scores s_j, x_j = s_j - max s, e_j = exp(x_j), S = sum e, w_j = e_j / S the output is out = sum_j w_j v_j. A kernel whose
score j is off by d_j (an absolute error of the exponential's argument = a relative error of e_j) computes weights w_j (1 + d_j) / sum_i w_i (1 + d_i), so

    |out' - out| = |sum_j w_j d_j (v_j - out)| / (1 + sum w d) <= sum_j w_j |d_j| |v_j - out|                                        (*)

to first order: an error common to all scores of a row cancels, and so does the error of a key that holds all the weight. (*) is evaluated term by term
for every case of at most 1024 keys. Beyond that (the 64 x 64 global grid alone), to keep it a matrix product, the row's top key is taken out exactly and the rest
is split at the key mean c of v: w_top d_top |v_top - out| + sum_{j != top} w_j d_j (|v_j - c| + |c - out|), which is no smaller.
d_j is the sum of

  score, MFMA kernels  D exact fp16 x fp16 products accumulated in fp32 by v_mfma_f32_16x16x16_f16. How an addition inside an fp16 MFMA rounds is not documented,
                 so each is MODELLED as off by at most one fp32 ulp (2 u), in any order: 2 D u sum |q k| (times the scale); the addition of a product that is
                 exactly 0 is exact whatever the rounding, so D counts the products that are not 0 (`_nnz`: a one-hot query costs nothing). What follows is plain fp32:
                 full_attention   acc * scale_log2e - m: the constant (log2 e rounded, sqrtf, the division: 3 u), the product (u): 4 u |s_j|; the subtraction u |x_j|.
                 relpos           (fmaf(acc, scale, rel_h) + rel_w) * LOG2E - m: scale = 1 / sqrtf(D) (2 u |q.k scale|), the FMA (u |q.k scale + rel_h|), the
                                  addition (u |s_j|), LOG2E and its product (2 u |s_j|), the subtraction (u |x_j|). rel_h and rel_w are MFMA dot products of the
                                  unscaled q with a table row, modelled alike.
  score, small_head    a serial chain of D FMAs (D u sum |q k| scale, plain fp32, no model), scale = 1 / sqrtf(D) and its product (3 u |s_j|), the subtraction.
  exponential    exp2f / __expf MODELLED as in encoder_ops_ref: X_j = (|x_j| + 4) 2^-23.
On the numerator alone:
  fp16 probabilities   the MFMA kernels round each p_j to fp16 before P.V while `sum` adds the unrounded p_j: half an fp16 ulp of p_j, i.e. a relative 2^-12 ..
                 2^-11 per weight, an absolute 2^-25 per key below the fp16 normal range, and p_j itself where p_j < 2^-25 (it rounds to 0). In relpos p_j is
                 taken against the running maximum m_t of its 64-key tile and scaled down by the later alphas (exp(m_t - m) <= 1) with its rounding error.
                 THIS TERM AND THE HALF ULP OF THE fp16 STORE DECIDE ALMOST EVERY CASE (a planted row has p = 1 exactly and is decided by the store alone).
  P.V            MFMA kernels: one accumulator chain per 16 output dims over ceil(nkeys / 16) MFMAs in program order (the accumulator is the data dependence),
                 each MODELLED as 16 additions off by 2 u in any order: key j passes through its own MFMA and every later one, 2 u cnt_j e_j |v_j| with
                 cnt_j the keys of those MFMAs whose fp16 p is not 0 (adding 0 is exact). small_head: a chain of ceil(Tk / 64) FMAs per lane and 6 butterfly
                 levels, plain fp32.
  rescale        relpos multiplies o and sum by the same alpha = exp2f(m_old - m_new) per key tile. What alpha multiplies is what the EARLIER tiles contributed,
                 so only the part of its error common to all keys cancels: the weight of key j passes through the alpha of every later tile, each a native
                 exponential off by (|dm| + 4) 2^-23 under the model (alpha = exp2f(0) = 1 exactly where the running maximum does not rise). The |dm| parts
                 telescope into m - m_t, which with the key's own |s_j - m_t| is the |x_j| already in X_j; the 4 2^-23 per later tile with a rising maximum
                 is added to X_j (the exponential's share). One rounding of the product per tile on each side (o, sum) remains.
On the denominator alone: the sum of nkeys positive terms in any order and the two shuffles, (nkeys + 2) u (small_head: ceil(Tk / 64) + 6). Then the reciprocal,
the product (3 u) and the fp16 store.

The two MODELS (the exponential, the 2 u per MFMA addition) cannot be verified without the hardware: every case must keep each model's share of its bound at or
below a tenth (`_core` asserts it, test_attn_ops_cpu.py asserts it for every GPU case). V = 1 + randn / 4 everywhere, so no output cancels. At more than 1024
keys the any-order P.V term alone would be a third of a diffuse row's bound (2 u 4096 = 4.9e-4 against a half ulp of 2.4e-4 .. 4.9e-4), so the diffuse and
late cases at such sizes let the scores rise along the keys by 20 (the weight sits at the end of the chain, cnt_j small where w_j is not; the ramp's own
product is in the modelled score error, which V = 1 + randn / 8 halves there).

The resize. The kernel computes the source coordinate in fp32: fy = max((y + 0.5) fl(sh / H) - 0.5, 0) (the division, the product and the subtraction, fused or
not: within 3 u (sh + 1) =: ey of the exact coordinate), y0 = min((int) fy, sh - 1), ly = fy - y0 (exact). The bilinear surface is continuous across cells, so a
coordinate off by ey moves the value by at most ey times the largest vertical difference of neighbouring source pixels within two rows / columns of the cell
(likewise ex along x), and the four-term blend (1 - ly) ((1 - lx) a + lx b) + ly (...) adds at most 8 u max(|a|, |b|, |c|, |d|) (seven roundings). The mask must
equal ref > thr on every pixel whose reference is farther from the threshold than this bound, and also where the bound is 0 (a flat zero neighbourhood: the kernel's
value is then exactly the reference).
"""
import functools
import math

import numpy as np
import torch

from encoder_ops_ref import _exp_model, round16, with_store16  # noqa: F401
from llm_ops_ref import SECOND, U, f64, half_ulp16, ratio  # noqa: F401

A_K, B_Q = 32.0, 8.0           # a planted key is A_K e_n, its query B_Q e_n: score 256 / sqrt(D) >= 28.6, every other key's below 1
MANY_KEYS = 1024               # above: the ramp of the docstring


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _v(g, *shape):
    return 1 + 0.25 * _rn(g, *shape)


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------------------------
def _core(s, Dn, Dm, v, kind, exact=True, tail=None, parts=False):
    """s, Dn, Dm [G, Tq, Tk] (scores, their plain and modelled error without u |x|), v [G, Tk, Dh]; kind full / relpos / small / unet; exact: (*) term by term
    -> out [G, Tq, Dh], bound, the largest share of the exponential model and of the MFMA model in it.
    kind unet (csrc/attention_core.h; unet_attn_ref.py lists its terms) is relpos' online softmax with the score arithmetic of that kernel; `tail` [G, Tq, 1]: keys
    with a non-zero fp16 probability that the same P.V accumulator takes in after this segment's; `parts`: -> (out, plain, model, ex, S) without SECOND and the store"""
    Tk, Dh = s.shape[-1], v.shape[-1]
    m = s.max(-1, keepdim=True).values
    x = s - m
    e = torch.exp(x)
    S = e.sum(-1, keepdim=True)
    w = e / S
    out = w @ v
    va, c = v.abs(), v.mean(-2, keepdim=True)
    top = w.argmax(-1, keepdim=True)
    dtop = (torch.gather(v, 1, top.expand(-1, -1, Dh)) - out).abs()
    dc, vc = (out - c).abs(), (v - c).abs()

    rows = max(1, (1 << 22) // (Tk * Dh))

    def lin(delta):                                     # (*) of the docstring: term by term (a few query rows at a time), or the split
        W = w * delta
        if exact:
            return torch.stack([torch.cat([(W[g, i:i + rows].unsqueeze(-1) * (v[g].unsqueeze(0) - out[g, i:i + rows].unsqueeze(1)).abs()).sum(1)
                                           for i in range(0, W.shape[1], rows)]) for g in range(len(W))])
        W0 = W.scatter(-1, top, 0.0)
        return torch.gather(W, -1, top) * dtop + W0 @ vc + dc * W0.sum(-1, keepdim=True)

    wv, oa, nl = w @ va, out.abs(), -(-Tk // 64)
    X = _exp_model(x)
    if kind == "small":
        plain = lin(Dn + U * x.abs()) + (nl + 6) * U * (wv + oa) + 3 * U * oa
        model = torch.zeros_like(out)
    else:
        if kind in ("relpos", "unet"):                  # p is rounded against the running maximum of its tile
            pad = nl * 64 - Tk
            sp = torch.nn.functional.pad(s, (0, pad), value=-math.inf) if pad else s
            rm = torch.cummax(sp.reshape(*s.shape[:-1], nl, 64).max(-1).values, -1).values
            mt = rm.repeat_interleave(64, -1)[..., :Tk]
            rise = torch.nn.functional.pad((rm[..., 1:] > rm[..., :-1]).double(), (0, 1))      # [.., t]: the running maximum rises entering tile t + 1
            X = X + 4 * 2.0 ** -23 * rise.flip(-1).cumsum(-1).flip(-1).repeat_interleave(64, -1)[..., :Tk]      # the alphas a key's weight passes through
        else:
            mt = m.expand_as(s)
        if kind == "unet":                              # fl(m_t c) is rounded per tile and alpha's exponent is not the difference of two of them (unet_attn_ref.py)
            Dn = Dn + U * (mt.abs() + x.abs()) + 3 * U * (m - mt)
        et = torch.exp(s - mt) * 1.001
        nt = -(-Tk // 16)
        nz = torch.nn.functional.pad((et >= 2.0 ** -25).double(), (0, nt * 16 - Tk)).reshape(*s.shape[:-1], nt, 16).sum(-1)      # keys per MFMA whose fp16 p is not 0
        cnt = nz.flip(-1).cumsum(-1).flip(-1).repeat_interleave(16, -1)[..., :Tk]
        if tail is not None:
            cnt = cnt + tail
        model = lin(Dm) + 2 * U * ((w * cnt) @ va)
        h = torch.minimum(et, half_ulp16(et)) * torch.exp(mt - m)
        plain = lin(Dn + U * x.abs()) + (h @ va) / S + (Tk + 5) * U * oa
        if kind in ("relpos", "unet"):
            plain = plain + nl * U * (wv + oa)
    ex = lin(X)
    if parts:
        return out, plain, model, ex, S
    total = with_store16(out, SECOND * (plain + model + ex))
    return out, total, float((SECOND * ex / total).max()), float((SECOND * model / total).max())


def _nnz(a, b):
    """the number of products of a . b that are not 0, per (row of a, row of b)"""
    return (a != 0).double() @ (b != 0).double().transpose(-1, -2)


def _check_shares(shares, what):
    assert shares[0] <= 0.1 and shares[1] <= 0.1, f"{what}: the modelled exponential / MFMA take {shares[0]:.3f} / {shares[1]:.3f} of the bound (a tenth at most)"
    return shares


# ---- ia2p_attention_full -----------------------------------------------------------------------------------------------------------------------------------------
def full_attention(qkv, bias_k, bias_v, B, T, heads, D):
    """qkv fp16 [B T, 3 heads D], bias_k / bias_v fp16 [heads D] or None -> (out [B T, heads D], bound, shares)"""
    x = f64(qkv).reshape(B, T, 3, heads, D).permute(2, 0, 3, 1, 4).reshape(3, B * heads, T, D)
    q, k, v = x[0], x[1], x[2]
    if bias_k is not None:
        rep = lambda t: f64(t).reshape(1, heads, 1, D).expand(B, heads, 1, D).reshape(B * heads, 1, D)      # noqa: E731
        k, v = torch.cat([k, rep(bias_k)], 1), torch.cat([v, rep(bias_v)], 1)
    scale = 1.0 / math.sqrt(D)
    s = (q @ k.transpose(1, 2)) * scale
    Dm = 2 * U * scale * _nnz(q, k) * (q.abs() @ k.abs().transpose(1, 2))
    out, bound, es, ms = _core(s, 4 * U * s.abs(), Dm, v, "full")
    fold = lambda t: t.reshape(B, heads, T, D).permute(0, 2, 1, 3).reshape(B * T, heads * D)      # noqa: E731
    return fold(out), fold(bound), _check_shares((es, ms), "full_attention")


# ---- ia2p_attention_window_relpos / ia2p_attention_global_relpos -------------------------------------------------------------------------------------------------
def rectangles(gh, gw, Sh, Sw):
    """per rectangle of the grid: (wy, wx, local index of its real positions, their grid index)"""
    loc = torch.arange(Sh * Sw)
    lh, lw = loc // Sw, loc % Sw
    for wy in range(-(-gh // Sh)):
        for wx in range(-(-gw // Sw)):
            y, xx = wy * Sh + lh, wx * Sw + lw
            real = (y < gh) & (xx < gw)
            yield wy, wx, loc[real], (y * gw + xx)[real]


def relpos_attention(qkv, bias, rel_h, rel_w, B, gh, gw, heads, D, window):
    """qkv fp16 [B gh gw, 3 heads D], bias fp16 [3 heads D] (None: global), rel_h [2 Sh - 1, D], rel_w [2 Sw - 1, D]; window 0: one rectangle, the grid
    -> (out [B gh gw, heads D], bound, shares). Written rectangle by rectangle with the kernel's index arithmetic; positions past the grid are keys that carry
    the bias' k / v and are no queries."""
    Sh, Sw = (window, window) if window else (gh, gw)
    nk, scale = Sh * Sw, 1.0 / math.sqrt(D)
    x = f64(qkv).reshape(B, gh * gw, 3, heads, D)
    Rh, Rw = f64(rel_h), f64(rel_w)
    out, bound = torch.zeros(B, gh * gw, heads, D, dtype=torch.float64), torch.zeros(B, gh * gw, heads, D, dtype=torch.float64)
    es = ms = 0.0
    kh, kw = torch.arange(nk) // Sw, torch.arange(nk) % Sw
    step = max(1, (1 << 21) // (heads * nk))
    for b in range(B):
        for wy, wx, loc, idx in rectangles(gh, gw, Sh, Sw):
            if len(loc) < nk:
                bq = f64(bias).reshape(3, heads, 1, D)
                k, v = bq[1].expand(heads, nk, D).clone(), bq[2].expand(heads, nk, D).clone()
            else:
                k, v = torch.empty(heads, nk, D, dtype=torch.float64), torch.empty(heads, nk, D, dtype=torch.float64)
            k[:, loc], v[:, loc] = x[b, idx, 1].transpose(0, 1), x[b, idx, 2].transpose(0, 1)
            qa = x[b, idx, 0].transpose(0, 1)                                          # [heads, nq, D]
            for i0 in range(0, len(loc), step):
                q, ql = qa[:, i0:i0 + step], loc[i0:i0 + step]
                ih = ((ql // Sw)[:, None] - kh[None, :] + Sh - 1).unsqueeze(0).expand(heads, -1, -1)
                iw = ((ql % Sw)[:, None] - kw[None, :] + Sw - 1).unsqueeze(0).expand(heads, -1, -1)
                qk = (q @ k.transpose(1, 2)) * scale
                bh, bw = torch.gather(q @ Rh.t(), 2, ih), torch.gather(q @ Rw.t(), 2, iw)
                a1 = qk + bh
                s = a1 + bw
                Dn = U * (2 * qk.abs() + a1.abs() + 3 * s.abs())
                Dm = 2 * U * (scale * _nnz(q, k) * (q.abs() @ k.abs().transpose(1, 2)) + torch.gather(_nnz(q, Rh) * (q.abs() @ Rh.abs().t()), 2, ih)
                              + torch.gather(_nnz(q, Rw) * (q.abs() @ Rw.abs().t()), 2, iw))
                o, bd, e1, m1 = _core(s, Dn, Dm, v, "relpos", exact=nk <= MANY_KEYS)
                out[b, idx[i0:i0 + step]], bound[b, idx[i0:i0 + step]] = o.transpose(0, 1), bd.transpose(0, 1)
                es, ms = max(es, e1), max(ms, m1)
    return out.reshape(B * gh * gw, heads * D), bound.reshape(B * gh * gw, heads * D), _check_shares((es, ms), "relpos_attention")


def relpos_lds_bytes(D, Sh, Sw):
    """the dynamic LDS of a relpos launch as csrc/sam.hip lays it out: K tile [64][D + 4] and V tile [D][64 + 4] in fp16, 64 packed key positions, and the
    fp32 bias rows of 64 queries [64][Sh + Sw + 1]"""
    return 64 * (D + 4) * 2 + D * (64 + 4) * 2 + 64 * 4 + 64 * (Sh + Sw + 1) * 4


THIN_GH = 3


def thin_grid(D):
    """the widest [THIN_GH, gw] grid whose launch fits 64 KiB of LDS by `relpos_lds_bytes` (the GPU test finds the same by calling the entry point)"""
    gw = 1
    while relpos_lds_bytes(D, THIN_GH, gw + 1) <= 64 * 1024:
        gw += 1
    return THIN_GH, gw


# ---- ia2p_attention_small_head -----------------------------------------------------------------------------------------------------------------------------------
def small_head_attention(q, k, v, heads):
    """q fp16 [B, Tq, heads D], k / v fp16 [B, Tk, heads D] -> (out as q, bound, shares): no MFMA, its share is 0"""
    B, Tq, H = q.shape
    D = H // heads
    f = lambda t: f64(t).reshape(B, -1, heads, D).transpose(1, 2).reshape(B * heads, -1, D)      # noqa: E731
    qq, kk, vv = f(q), f(k), f(v)
    scale = 1.0 / math.sqrt(D)
    s = (qq @ kk.transpose(1, 2)) * scale
    Dn = D * U * scale * (qq.abs() @ kk.abs().transpose(1, 2)) + 3 * U * s.abs()
    out, bound, es, ms = _core(s, Dn, torch.zeros_like(s), vv, "small")
    fold = lambda t: t.reshape(B, heads, Tq, D).transpose(1, 2).reshape(B, Tq, H)      # noqa: E731
    return fold(out), fold(bound), _check_shares((es, ms), "small_head_attention")


# ---- the cases of the GPU tests (built on the CPU; test_attn_ops_cpu.py checks the two shares for every one) ---------------------------------------------------
def _slots(nq, edges):
    """query i plants edges[i % len]: -> (slot of every query, the unique edges in order)"""
    edges = list(dict.fromkeys(int(e) for e in edges))
    return torch.arange(nq) % len(edges), edges


def _onehot(slot, D, amp):
    return amp * torch.nn.functional.one_hot(slot, D).double()


FULL_D = (64, 80)
FULL_T = ((1, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0), (255, 0), (256, 0), (257, 0), (272, 0), (16, 1), (32, 1), (229, 1), (256, 1), (271, 1))
FULL_B, FULL_HEADS = 2, 3


@functools.lru_cache(maxsize=None)
def full_case(family, T, bias, D):
    """-> (qkv, bias_k, bias_v, want): diffuse q, k ~ N(0, 1); planted: query i leads on key edges[i % n] of {0, 15, 16, T - 1, the bias row} by 28 or more
    (want = that key's value row per output row, the bias' v row where it is the bias row)"""
    B, heads, g = FULL_B, FULL_HEADS, gen(1000 * D + 2 * T + bias)
    q, k, v = _rn(g, B, T, heads, D), _rn(g, B, T, heads, D), _v(g, B, T, heads, D)
    bk, bv = (_rn(g, heads, D), _v(g, heads, D)) if bias else (None, None)
    want = None
    if family == "planted":
        slot, edges = _slots(T, [e for e in (0, 15, 16, T - 1) if e < T] + ([T] if bias else []))
        k = 0.05 * k
        q = _onehot(slot, D, B_Q).reshape(1, T, 1, D).expand(B, T, heads, D)
        vall = torch.cat([v, bv.reshape(1, 1, heads, D).expand(B, 1, heads, D)], 1) if bias else v
        for n, e in enumerate(edges):
            if e < T:
                k[:, e] = _onehot(torch.tensor(n), D, A_K)
            else:
                bk = _onehot(torch.tensor(n), D, A_K).expand(heads, D).clone()
        want = vall.half().double()[:, torch.tensor(edges)[slot]].reshape(B * T, heads * D)
    qkv = torch.stack([q, k, v], 2).reshape(B * T, 3 * heads * D).half()
    return qkv, None if bk is None else bk.reshape(-1).half(), None if bv is None else bv.reshape(-1).half(), want


def full_cases():
    for D in FULL_D:
        for T, bias in FULL_T:
            for family in ("diffuse", "planted"):
                yield family, T, bias, D


@functools.lru_cache(maxsize=None)
def full_ref(family, T, bias, D):
    qkv, bk, bv, _ = full_case(family, T, bias, D)
    return full_attention(qkv, bk, bv, FULL_B, T, FULL_HEADS, D)


GLOBAL_GRIDS = ((1, 1), (5, 5), (9, 7), (8, 8), (13, 5), (1, 70), (70, 1), (28, 12), (64, 64), "thin")
WINDOW_CASES = ((14, 20, 20, 80), (14, 28, 28, 80), (14, 5, 20, 80), (14, 20, 33, 80), (14, 64, 64, 80), (16, 32, 20, 80), (7, 20, 20, 80), (1, 3, 5, 80),
                (14, 20, 33, 64), (7, 20, 20, 64))
DH0, DW0 = 2, -3


def relpos_dims(gh, gw, window=0):
    """(B, heads): 2 x 3 where the block decode is at stake, 1 x 1 at the large key counts (a global grid of more than 450 keys) and on the 64 x 64 grid"""
    return (1, 1) if gh * gw > (1024 if window else 450) else (2, 3)


def table_offsets(Sh, Sw):
    """the planted offset of the tables family (an axis too short for it keeps 0)"""
    return (DH0 if Sh > abs(DH0) else 0), (DW0 if Sw > abs(DW0) else 0)


@functools.lru_cache(maxsize=None)
def relpos_case(family, window, gh, gw, D):
    """-> (qkv, bias, rel_h, rel_w, want). Families:
    diffuse  q ~ N(0, 0.3^2) (the three MFMA dot products of a score are modelled: a larger q takes their share past a tenth), k ~ N(0, 1), tables N(0, 0.07^2); above MANY_KEYS keys the scores also rise by 20 along the keys and V = 1 + randn / 8 (docstring)
    planted  query i of a rectangle leads by 26 or more on the real key edges[i % n] of the rectangle's keys {0, 63, 64, nkeys - 1} (through q . k)
    tables   one relative-position entry dominant (above MANY_KEYS keys the six queries with no target on either axis plant key 64 through q . k instead): the key at (qh - dh0, qw - dw0) leads by 22 per axis (as `_dominant_case` of test_sam_gpu.py, at 8 x 2.75), dh0 = 2, dw0 = -3
    late     the first 64 keys of every rectangle score about 120 below the later ones
    pad      (windows) the bias' k row leads: every query of a rectangle with pad keys returns the bias' v row, queries of full rectangles do not"""
    B, heads = relpos_dims(gh, gw, window)
    Sh, Sw = (window, window) if window else (gh, gw)
    nk, P, g = Sh * Sw, gh * gw, gen(100000 * window + 1000 * gh + 10 * gw + D)
    q, k, v = _rn(g, B, P, heads, D), _rn(g, B, P, heads, D), _v(g, B, P, heads, D)
    bias = torch.stack([_rn(g, heads, D), 0.5 * _rn(g, heads, D), _v(g, heads, D)])
    rh, rw = 0.1 * _rn(g, 2 * Sh - 1, D), 0.1 * _rn(g, 2 * Sw - 1, D)
    want = torch.full((B, P, heads, D), float("nan"), dtype=torch.float64)
    ramp = nk > MANY_KEYS and family in ("diffuse", "late")
    if ramp:
        v = 1 + 0.5 * (v - 1)
    if family == "diffuse":
        q, rh, rw = 0.3 * q, 0.7 * rh, 0.7 * rw
    if family in ("planted", "pad", "tables"):
        k, rh, rw = 0.05 * k, 0.2 * rh, 0.2 * rw
    if family == "planted":
        q = torch.zeros_like(q)
        for wy, wx, loc, idx in rectangles(gh, gw, Sh, Sw):
            real = {int(a): int(b) for a, b in zip(loc, idx)}
            slot, edges = _slots(len(loc), [e for e in (0, 63, 64, nk - 1) if e in real])
            q[:, idx] = _onehot(slot, D, B_Q).reshape(1, -1, 1, D)
            for n, e in enumerate(edges):
                k[:, real[e]] = _onehot(torch.tensor(n), D, A_K)
            want[:, idx] = v.half().double()[:, torch.tensor([real[e] for e in edges])[slot]]
    elif family == "pad":
        q = _onehot(torch.zeros(P, dtype=torch.long), D, B_Q).reshape(1, P, 1, D).expand(B, P, heads, D)
        bias[1] = _onehot(torch.tensor(0), D, A_K)
        for wy, wx, loc, idx in rectangles(gh, gw, Sh, Sw):
            if len(loc) < nk:
                want[:, idx] = bias[2].half().double()
    elif family == "tables":
        dh0, dw0 = table_offsets(Sh, Sw)
        q, rh, rw = 0.1 * q, torch.zeros_like(rh), torch.zeros_like(rw)
        q[..., 0] = 8.0
        if nk > MANY_KEYS:      # the queries with no target on either axis would weigh all keys alike (a modelled P.V chain of nk additions): they plant key 64 through q . k
            lost = [a for a in range(nk) if not 0 <= a // Sw - dh0 < Sh and not 0 <= a % Sw - dw0 < Sw]
            q[:, lost] = _onehot(torch.tensor(1), D, B_Q)
            k[:, 64] = _onehot(torch.tensor(1), D, A_K)
            want[:, lost] = v.half().double()[:, 64:65]
        if dh0:
            rh[dh0 + Sh - 1, 0] = 2.75
        if dw0:
            rw[dw0 + Sw - 1, 0] = 2.75
        vh = v.half().double()
        for wy, wx, loc, idx in rectangles(gh, gw, Sh, Sw):
            real = {int(a): int(b) for a, b in zip(loc, idx)}
            for a, b in real.items():
                th, tw = a // Sw - dh0, a % Sw - dw0
                if 0 <= th < Sh and 0 <= tw < Sw and th * Sw + tw in real and (dh0 or Sh == 1) and (dw0 or Sw == 1):
                    want[:, b] = vh[:, real[th * Sw + tw]]
    elif family == "late":
        q, k, rh, rw = 1 + 0.05 * q, 0.5 * k, 0.2 * rh, 0.2 * rw
        for wy, wx, loc, idx in rectangles(gh, gw, Sh, Sw):
            k[:, idx[loc < 64]] = -120.0 * math.sqrt(D) / D
    if ramp:
        q[..., 0] = 4.0
        k[..., 0] = (20.0 * math.sqrt(D) / 4.0) * (torch.arange(P).double() / P).reshape(1, P, 1)
    qkv = torch.stack([q, k, v], 2).reshape(B * P, 3 * heads * D).half()
    return qkv, bias.reshape(-1).half(), rh.half(), rw.half(), want.reshape(B * P, heads * D)


def global_grid(grid, D):
    return thin_grid(D) if grid == "thin" else grid


def global_cases():
    """(family, gh, gw, D)"""
    for D in (64, 80):
        for grid in GLOBAL_GRIDS:
            gh, gw = global_grid(grid, D)
            for family in ("diffuse", "planted", "tables", "late"):
                if family == "late" and gh * gw <= 64 or family == "tables" and table_offsets(gh, gw) == (0, 0):
                    continue
                yield family, gh, gw, D


def window_cases():
    for window, gh, gw, D in WINDOW_CASES:
        for family in ("diffuse", "planted", "pad"):
            yield family, window, gh, gw, D


@functools.lru_cache(maxsize=None)
def relpos_ref(family, window, gh, gw, D):
    qkv, bias, rh, rw, _ = relpos_case(family, window, gh, gw, D)
    B, heads = relpos_dims(gh, gw, window)
    return relpos_attention(qkv, bias if window else None, rh, rw, B, gh, gw, heads, D, window)


SMALL_D = (16, 32)
SMALL_SHAPES = ((1, 1, 1, 1), (1, 1, 63, 1), (1, 3, 64, 1), (2, 7, 65, 8), (1, 7, 4096, 8), (1, 4096, 7, 8))      # (B, Tq, Tk, heads)


@functools.lru_cache(maxsize=None)
def small_case(family, B, Tq, Tk, heads, D):
    """-> (q, k, v, want); planted: query i leads on key edges[i % n] of {0, 63, 64, Tk - 1}"""
    g = gen(10000 * D + 100 * Tq + Tk + heads)
    q, k, v = _rn(g, B, Tq, heads, D), _rn(g, B, Tk, heads, D), _v(g, B, Tk, heads, D)
    want = None
    if family == "planted":
        slot, edges = _slots(Tq, [e for e in (0, 63, 64, Tk - 1) if e < Tk])
        k = 0.05 * k
        q = _onehot(slot, D, B_Q).reshape(1, Tq, 1, D).expand(B, Tq, heads, D)
        for n, e in enumerate(edges):
            k[:, e] = _onehot(torch.tensor(n), D, A_K)
        want = v.half().double()[:, torch.tensor(edges)[slot]].reshape(B, Tq, heads * D)
    h = lambda t: t.reshape(B, -1, heads * D).half()      # noqa: E731
    return h(q), h(k), h(v), want


def small_cases():
    for D in SMALL_D:
        for shape in SMALL_SHAPES:
            for family in ("diffuse", "planted"):
                yield (family, *shape, D)


@functools.lru_cache(maxsize=None)
def small_ref(family, B, Tq, Tk, heads, D):
    q, k, v, _ = small_case(family, B, Tq, Tk, heads, D)
    return small_head_attention(q, k, v, heads)


# ---- ia2p_mask_upsample_threshold ----------------------------------------------------------------------------------------------------------------------------------
def bilinear_resize(src, sh, sw, H, W):
    """src fp32 [n, rows >= sh, ld >= sw] (the crop [sh, sw] is resized) -> (ref fp64 [n, H, W], bound): the kernel's index arithmetic in fp64, the bound of the
    docstring"""
    s = f64(src)[:, :sh, :sw]

    def axis(n_out, n_src):
        c = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_src / n_out) - 0.5).clamp_min(0.0)
        i0 = c.floor().long().clamp_max(n_src - 1)
        return c - i0, i0, (i0 + 1).clamp_max(n_src - 1)

    ly, y0, y1 = axis(H, sh)
    lx, x0, x1 = axis(W, sw)
    ly, lx = ly.reshape(1, H, 1), lx.reshape(1, 1, W)
    a, b, c, d = s[:, y0][:, :, x0], s[:, y0][:, :, x1], s[:, y1][:, :, x0], s[:, y1][:, :, x1]
    ref = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)
    gy, gx = torch.zeros_like(s), torch.zeros_like(s)
    gy[:, :-1], gx[:, :, :-1] = (s[:, 1:] - s[:, :-1]).abs(), (s[:, :, 1:] - s[:, :, :-1]).abs()
    pool = lambda t: torch.nn.functional.max_pool2d(t[None], 5, 1, 2)[0]      # noqa: E731
    Gy, Gx = pool(gy)[:, y0][:, :, x0], pool(gx)[:, y0][:, :, x0]
    M = torch.stack([a, b, c, d]).abs().max(0).values
    return ref, SECOND * (3 * U * (sh + 1) * Gy + 3 * U * (sw + 1) * Gx + 8 * U * M)


def sure_pixels(ref, bound, thr):
    """where the mask is decided: the reference farther from the threshold than its bound, or a bound of 0 (the kernel's value is the reference)"""
    thr = float(np.float32(thr))
    return ((ref - thr).abs() > bound) | (bound == 0)


UPSAMPLE_CASES = (("80to320", 2, 80, 80, 80, 80, 320, 320), ("7x5to600x257", 2, 7, 5, 7, 5, 600, 257), ("down", 2, 64, 64, 64, 64, 16, 24), ("1x1", 2, 1, 1, 1, 1, 9, 9),
                  ("crop", 3, 40, 72, 48, 80, 50, 90))      # (name, n, sh, sw, rows, ld, H, W)
UPSAMPLE_THR = (0.0, 0.37)


@functools.lru_cache(maxsize=None)
def upsample_case(name):
    """fp32 [n, rows, ld]: N(0, 1) logits; image 0 of 80to320 holds a 16 x 16 block of exact zeros (a `>=` in place of `>` shows at threshold 0); the 1 x 1
    sources are 1.5 and -0.75"""
    _, n, sh, sw, rows, ld, H, W = next(c for c in UPSAMPLE_CASES if c[0] == name)
    x = torch.randn(n, rows, ld, generator=gen(len(name) + H)).float()
    if name == "80to320":
        x[0, 30:46, 20:36] = 0.0
    if name == "1x1":
        x[:, 0, 0] = torch.tensor([1.5, -0.75])
    return x


# ---- ia2p_mask_morph -------------------------------------------------------------------------------------------------------------------------------------------------
def morph(img, k, dilate):
    """uint8 [H, W] numpy -> the k x k minimum (erode) or maximum (dilate) over offsets -(k / 2) .. k - k / 2 - 1 on both axes, pixels outside ignored"""
    op, fill = (np.maximum, 0) if dilate else (np.minimum, 255)
    out = np.asarray(img, dtype=np.uint8)
    for ax in (1, 0):
        n = out.shape[ax]
        acc = np.full_like(out, fill)
        for off in range(max(-(k // 2), -(n - 1)), min(k - k // 2 - 1, n - 1) + 1):
            dst, src = [slice(None)] * 2, [slice(None)] * 2
            dst[ax], src[ax] = slice(max(0, -off), n - max(0, off)), slice(max(0, off), n - max(0, -off))
            acc[tuple(dst)] = op(acc[tuple(dst)], out[tuple(src)])
        out = acc
    return out


MORPH_W, MORPH_H, MORPH_K = (255, 256, 257, 600), (1, 37), (1, 2, 7, 10, 700)


def morph_masks(H, W, seed):
    """random masks (sparse set, sparse clear, half) and masks whose only set / only clear pixel is at a corner or on either side of column 255 / 256"""
    rng = np.random.default_rng(seed)
    masks = [np.where(rng.random((H, W)) < p, 255, 0).astype(np.uint8) for p in (0.02, 0.98, 0.5)]
    for y, x in {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 254), (H // 2, 255), (H // 2, 256), (H - 1, 257)}:
        if x < W:
            for base in (0, 255):
                m = np.full((H, W), base, np.uint8)
                m[y, x] = 255 - base
                masks.append(m)
    return masks
