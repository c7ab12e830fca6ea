"""fp64 references of the LLM decode and prefill operations, and next to each the error bound its HIP kernel must meet.

Every reference takes exactly the bits the kernel is given (fp16 weights, gamma and cache rows; fp32 x, q, eps, scale and inv_freq; for the 4-bit format the
codes, the fp32 absmax and the fp32 codebook, whose products are exact in fp64) and computes in float64. Every bound is derived from operation counts, never
from what a kernel returned. Notation: u = 2^-24, the unit roundoff of fp32; fl(.) a value as computed in fp32.

The building blocks (to first order; SECOND covers the second-order terms, which are below K u <= 14336 * 2^-24 < 1e-3 of the first-order ones):

  dot product   A sum of K products in fp32, in ANY order and with or without fused multiply-adds, is off by at most K u sum_i |x_i w_i|: a term passes through
                its own product and at most K - 1 additions. The kernels' K-splits (threads, lanes, waves, LDS) are orders of this kind; the 4-bit kernels scale
                a block's partial sum by absmax in the FMA that accumulates it, one more operation on a path that has fewer than K - 1 additions.
  RMSNorm fold  out = rstd * sum_i (x_i gamma_i) w_i, rstd = 1 / sqrt(sum x^2 / K + eps). sum x^2 has positive terms only: relative error K u, taken over in
                full (the square root would halve it); the division by K, the addition of eps, the square root and the reciprocal are correctly rounded: 4 u.
                The rounding of x_i gamma_i adds u to every term of the dot product, and the product with rstd one more u:
                  |fl(out) - out| <= u rstd ((K + 1) sum |x_i gamma_i w_i| + (K + 5) |sum x_i gamma_i w_i|).
  rotated pair  y1 = x1 cos a - x2 sin a, y2 = x2 cos a + x1 sin a with a = fl(pos * inv_freq[i]) (the fp32 product is the DEFINITION of the angle, here as in
                transformers; its cos and sin are taken in fp64): (|x1| + |x2|) (u a + 2^-21). The first term is a rounding of the angle product, the second
                covers cosf / sinf (2 ulp = 2^-22 each, on a factor of at most 1) and the two multiplies and the addition (3 u).
  fp16 output   the fp32 bound plus half an fp16 ulp at |ref| + bound (round to nearest, subnormals kept).
"""
import numpy as np
import torch

U = 2.0 ** -24
SECOND = 1.001
ATTN_SCALE = float(np.float32(0.08838834764831845))      # the kernels' `float scale`


def f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def half_ulp16(a):
    """half the spacing of fp16 at magnitude a (a >= 0): 2^(floor(log2 a) - 11), and 2^-25 in the subnormal range"""
    e = torch.floor(torch.log2(f64(a).clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 11)


def ratio(got, ref, bound):
    """max(err / bound) over the outputs (0 / 0 counts as 0; a non-finite output as inf)"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def inv_freq_torch(theta):
    """transformers `LlamaRotaryEmbedding` (default rope, head dim 128): computed with torch in fp32"""
    return 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.int64).float() / 128))


def unpack_q4(packed, absmax, codebook, N, K):
    """the exact weights of the 4-bit format: codebook[code] * absmax (fp32 x fp32: exact in fp64). packed: uint8 [N K / 2], weight 2 b in the low nibble of
    byte b and 2 b + 1 in the high one; absmax: fp32 [N K / 64]; codebook: 16 floats"""
    b = torch.as_tensor(packed).cpu().to(torch.int64).reshape(-1)
    codes = torch.stack([b & 15, b >> 4], dim=1).reshape(-1)
    cb = torch.tensor([float(np.float32(v)) for v in codebook], dtype=torch.float64)
    return (cb[codes].reshape(-1, 64) * f64(absmax).reshape(-1, 1)).reshape(N, K)


# ---- the GEMVs ---------------------------------------------------------------------------------------------------------------------------------------------
def gemv_sums(W, x, gamma=None, eps=0.0):
    """r [M, N] = rstd * (x gamma) . W^T in fp64 and the bound E [M, N] on fl(r) (the plain epilogue's output): K u sum |x w| without gamma (rstd = 1 is exact),
    the RMSNorm-fold bound above with it. Also rstd [M, 1]."""
    W, x = f64(W), f64(x)
    K = W.shape[1]
    if gamma is None:
        S, A = x @ W.t(), x.abs() @ W.abs().t()
        return S, SECOND * K * U * A, torch.ones(x.shape[0], 1, dtype=torch.float64)
    y = x * f64(gamma)
    rstd = 1.0 / torch.sqrt((x * x).sum(1, keepdim=True) / K + float(np.float32(eps)))
    S, A = y @ W.t(), y.abs() @ W.abs().t()
    return rstd * S, SECOND * U * rstd * ((K + 1) * A + (K + 5) * S.abs()), rstd


def gemv_plain(W, x, gamma=None, eps=0.0):
    """-> (out, bound) and, with gamma, (hid, bound): hid = fl(fl(x rstd) gamma), rstd's K + 4 roundings and the two products"""
    r, E, rstd = gemv_sums(W, x, gamma, eps)
    if gamma is None:
        return r, E, None, None
    hid = f64(x) * rstd * f64(gamma)
    return r, E, hid, SECOND * (W.shape[1] + 6) * U * hid.abs()


def gemv_resid(W, x, out0, gamma=None, eps=0.0):
    """out = out0 + r, one FMA: the bound of r and one rounding of the result"""
    r, E, _ = gemv_sums(W, x, gamma, eps)
    ref = f64(out0) + r
    return ref, E + U * ref.abs()


def gemv_swiglu(W, x, gamma=None, eps=0.0):
    """out[i] = silu(g_i) up_i with g = r[:I], up = r[I:] and their bounds Eg, Eu. To first order
         |d out| <= |silu'(g)| Eg |up| + |silu(g)| Eu + 8 u |out|,   silu'(g) = s (1 + g (1 - s)), s = sigmoid(g).
    The 8 u: expf within 2 ulp (4 u, and 1 + e takes over at most that), the addition, the division, the product with up, one spare."""
    r, E, _ = gemv_sums(W, x, gamma, eps)
    I = r.shape[1] // 2
    g, up, Eg, Eu = r[:, :I], r[:, I:], E[:, :I], E[:, I:]
    s = torch.sigmoid(g)
    ref = g * s * up
    return ref, (s * (1 + g * (1 - s))).abs() * Eg * up.abs() + (g * s).abs() * Eu + SECOND * 8 * U * ref.abs()


# ---- rotary embedding ----------------------------------------------------------------------------------------------------------------------------------------
def rope_angles(pos, inv_freq):
    """[len(pos), 64] fp64 values of the fp32 products float32(pos) * inv_freq[i]"""
    p = np.asarray(pos, dtype=np.float32).reshape(-1, 1)
    f = torch.as_tensor(inv_freq).detach().cpu().float().numpy().reshape(1, 64)
    a = p * f
    assert a.dtype == np.float32
    return torch.from_numpy(a.astype(np.float64))


def _rotate(x, E, ang):
    """x, E: [M, H] rows and the bound on each entry as it enters the rotation; ang [M, 64] -> rotated rows and their bound (inputs propagated to first order +
    the rotated-pair term)"""
    M, H = x.shape
    xs, Es = x.reshape(M, H // 128, 2, 64), E.reshape(M, H // 128, 2, 64)
    x1, x2, E1, E2 = xs[:, :, 0], xs[:, :, 1], Es[:, :, 0], Es[:, :, 1]
    a = ang.reshape(M, 1, 64)
    c, s = torch.cos(a), torch.sin(a)
    own = (x1.abs() + x2.abs()) * (U * a + 2.0 ** -21) * SECOND
    y = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=2).reshape(M, H)
    B = torch.stack([c.abs() * E1 + s.abs() * E2 + own, c.abs() * E2 + s.abs() * E1 + own], dim=2).reshape(M, H)
    return y, B


def gemv_qkv(W, x, pos, inv_freq, gamma=None, eps=0.0):
    """W [3 H, K] = q | k | v rows. -> dict of (ref, bound): q [M, H] fp32 (rotated); k, v [M, H], the fp16 cache rows at pos[m] (k rotated; v the rounded sum)"""
    r, E, _ = gemv_sums(W, x, gamma, eps)
    H = r.shape[1] // 3
    ang = rope_angles(pos, inv_freq)
    q, Bq = _rotate(r[:, :H], E[:, :H], ang)
    k, Bk = _rotate(r[:, H:2 * H], E[:, H:2 * H], ang)
    v, Bv = r[:, 2 * H:], E[:, 2 * H:]
    return {"q": (q, Bq), "k": (k, Bk + half_ulp16(k.abs() + Bk)), "v": (v, Bv + half_ulp16(v.abs() + Bv))}


def rope_rows(qkv, p0, inv_freq):
    """the prefill row kernel: qkv fp16 [T, 3 H] enters exactly, so q carries the rotated-pair term alone, k that and the fp16 rounding; v is a copy (bound 0)"""
    x = f64(qkv)
    T, H = x.shape[0], x.shape[1] // 3
    ang = rope_angles(np.arange(p0, p0 + T), inv_freq)
    zero = torch.zeros(T, H, dtype=torch.float64)
    q, Bq = _rotate(x[:, :H], zero, ang)
    k, Bk = _rotate(x[:, H:2 * H], zero, ang)
    return {"q": (q, Bq), "k": (k, Bk + half_ulp16(k.abs() + Bk)), "v": (x[:, 2 * H:], zero)}


# ---- attention -----------------------------------------------------------------------------------------------------------------------------------------------
def attention_row(q, kc, vc, fp16_out=False):
    """one query row q [H] fp32 against the keys / values kc, vc [nk, H] fp16, head dim 128: out [H] = softmax(scale q . k) v per head, and per channel c the bound
         (2 D + (nk + 16) u + 2^-20) sum_j p_j |v_jc|,   D = max_j [130 u scale sum_e |q_e k_je| + 2^-23 |s_j - m|]
    D bounds what reaches the argument of expf: the score (128 products of q_e scale and k_je, the scaling of q_e, one spare) and, twice (s_j and the maximum m),
    the rounding of their difference; e^x turns an absolute error of its argument into a relative one of its value, for numerator and denominator: 2 D.
    (nk + 16) u: the sums over the keys (P.V in 16 groups of nk / 16 and across the groups, the denominator in 256 partial sums). 2^-20: expf, the product p v,
    the division. With fp16_out the half ulp of the store."""
    q, kc, vc = f64(q), f64(kc), f64(vc)
    nk, H = kc.shape
    h = H // 128
    qh, kh, vh = q.reshape(h, 128), kc.reshape(nk, h, 128).transpose(0, 1), vc.reshape(nk, h, 128).transpose(0, 1)      # [h, nk, 128]
    s = ATTN_SCALE * torch.einsum("he,hje->hj", qh, kh)
    sa = ATTN_SCALE * torch.einsum("he,hje->hj", qh.abs(), kh.abs())
    m = s.max(dim=1, keepdim=True).values
    p = torch.softmax(s, dim=1)
    D = (130 * U * sa + 2.0 ** -23 * (s - m).abs()).max(dim=1, keepdim=True).values
    out = torch.einsum("hj,hjc->hc", p, vh)
    B = SECOND * (2 * D + (nk + 16) * U + 2.0 ** -20) * torch.einsum("hj,hjc->hc", p, vh.abs())
    out, B = out.reshape(H), B.reshape(H)
    return (out, B + half_ulp16(out.abs() + B)) if fp16_out else (out, B)


# ---- the other prefill row kernels ---------------------------------------------------------------------------------------------------------------------------
def rmsnorm_rows(x, gamma, eps):
    """y = fp16(fl(fl(x rstd) gamma)), x and gamma fp16: rstd's H + 4 roundings (sum of H squares of exact fp16 values, the four correctly rounded operations)
    and the two products, (H + 6) u |y|, then the fp16 rounding"""
    x = f64(x)
    H = x.shape[1]
    rstd = 1.0 / torch.sqrt((x * x).sum(1, keepdim=True) / H + float(np.float32(eps)))
    y = x * rstd * f64(gamma)
    B = SECOND * (H + 6) * U * y.abs()
    return y, B + half_ulp16(y.abs() + B)


def silu_mul_rows(gu):
    """act = fp16(silu(gate) up) of gu fp16 [T, 2 I] = gate | up, both exact: the 8 u of the SwiGLU epilogue, then the fp16 rounding"""
    gu = f64(gu)
    I = gu.shape[1] // 2
    g, up = gu[:, :I], gu[:, I:]
    y = g * torch.sigmoid(g) * up
    B = SECOND * 8 * U * y.abs()
    return y, B + half_ulp16(y.abs() + B)
