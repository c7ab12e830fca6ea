"""fp64 references of the small launches around the UNet -- CLIP text / prior stem, causal attention and pooling, VAE softmax and 1x1 convolution, ViT stem and
head projection, the SAM decoder's pieces, the UNet's embeddings, concats and the IP-Adapter attention map -- and next to each the error bound its HIP kernel
must meet. Written in the manner of llm_ops_ref.py, whose notation it keeps: u = 2^-24, SECOND covers second-order terms.

Every reference takes exactly the bits the kernel is given (fp16 tensors, fp32 scalars) and computes in float64. Every bound is derived from operation counts,
never from what a kernel returned. Pure data movement (patch_gather, pixel_shuffle2, concat, the weight rows of cat_rows, sam_take_col, ReLU) has no bound: the
tests hold it to torch.equal.

The building blocks:

  one operation  fp16(fl(a + b)), a and b fp16: one fp32 rounding, u |ref|, and half an fp16 ulp at |ref| + that. (The fp32 sum of two fp16 values is in fact
                 exact unless the smaller lies below 2^-13 of the larger, where it cannot move the fp16 result: the kernel's value is the correctly rounded
                 fp16 sum either way, and an fp16 addition rounds once.)
  sum, dot       K u sum |terms| for K terms in any order (llm_ops_ref). Products of two fp16 values are exact in fp32 (22 bits).
  LayerNorm      y = (x - mean) rstd g + b in fp32, two passes, over a row whose entries are already off by E_i (0 for fp16 inputs):
                   mean   d_m  = u sum |x| + u |mean| + mean(E)                     (H additions in any order: H u sum |x| / H; the division)
                   x-mean e_i  = u |x_i - mean| + d_m + E_i
                   var    d_v  = sum (2 |x_i - mean| e_i + e_i^2) / H + (H + 2) u var   (the squares, H additions, the division)
                   rstd   r    = (1 - d_v / (var + eps))^-1/2 - 1 + 3 u             (the addition of eps; rsqrtf within 1 ulp = 2 u)
                   y      |g| rstd (e_i + |x_i - mean| (r + 2 u)) + u |y|           (the products with rstd and g; the addition of b)
  row statistics {sum, sum of squares} over the fp16-ROUNDED outputs of a row of H: the reference sums its own correctly rounded row xr. A kernel whose fp32
                 value lies within B_i of the reference may store either neighbour where a rounding boundary lies within B_i: with lo_i = fp16(ref_i - B_i),
                 hi_i = fp16(ref_i + B_i) (rounding is monotonic) its fp16 value is in [lo_i, hi_i], off from xr_i by at most d_i = hi_i - lo_i (0 for most
                 entries). That is the term for legitimately differing rows:
                   sum    H u sum (|xr_i| + d_i) + sum d_i
                   sum^2  (H + 1) u sum (|xr_i| + d_i)^2 + sum d_i (2 |xr_i| + d_i)
  native exp     the kernels that use __expf / exp2 (causal_attention_small, softmax_rows, ip_attn_map): the error reaching the exponential's argument x turns
                 into a relative error D of its value; the exponential itself is MODELLED as off by X = (|x| + 4) 2^-23 relatively (one rounding of x log2(e)
                 and a 1-ulp hardware exp2, doubled). A normalised weight p_j = e_j / sum e then carries D_j + X_j + sum_i p_i (D_i + X_i) (its own and the
                 denominator's, a weighted mean) plus the roundings of the sum, the reciprocal and the product; an error of the row maximum is a common factor
                 and cancels. X cannot be verified without the hardware, so every case must keep its share of the bound below a tenth (`exp_share`, asserted
                 here): the fp16 half ulp and the summation terms decide each case.
  sinusoids      cos / sin of a = t f_k, f_k = exp(-ln(10000) k / half): in front of the angle the constant, its product with k and the division (3 u y,
                 y = ln(10000) k / half, an absolute error of expf's argument = a relative one of f), expf within 2 ulp (4 u) and the product with t (u):
                 |a| (3 u y + 5 u); cosf / sinf within 2 ulp of a value below 1: 2^-22.
  GELU           gelu_erf_f (csrc/common.h) = 0.5 x (1 + erf_as(x / sqrt 2)), erf_as the Abramowitz-Stegun 7.1.26 polynomial with a hardware reciprocal and a
                 native exponential: its accuracy is not derivable from operation counts. GELU_ERF_CPU is the largest |erf_as - erf| of the SAME polynomial in
                 numpy fp32 (`erf_poly32`) over every fp16 x in [-8, 8], measured on the CPU: 5.55e-7 (the 1.5e-7 of the formula and its fp32 roundings; test_encoder_ops_cpu.py measures it again). The device
                 differs from numpy by the reciprocal (1 ulp: 3 u through the polynomial, whose t-derivative stays below 1.3) and the exponential ((y + 4) 2^-23
                 e^-y <= 8 u): 11 u. Then 0.5 |x| (GELU_ERF_CPU + 11 u) + 4 u |gelu| (the scaling of x, 1 + erf, the two products) and the fp16 half ulp.
"""
import math

import numpy as np
import torch

from llm_ops_ref import SECOND, U, f64, half_ulp16, ratio  # noqa: F401

LN1E4 = math.log(10000.0)
GELU_ERF_CPU = 5.6e-7      # >= the measured 5.55e-7


def round16(x):
    """the correctly rounded fp16 values of an fp64 tensor, as fp64 (numpy converts double to half in one rounding)"""
    return torch.from_numpy(f64(x).numpy().astype(np.float16).astype(np.float64))


def with_store16(ref, B):
    """an fp32 bound B and the fp16 store"""
    return B + half_ulp16(ref.abs() + B)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- one operation and an fp16 store ---------------------------------------------------------------------------------------------------------------------
def add16(a, b):
    """fp16(fl(a + b)) -> (ref, bound, fp32 bound)"""
    ref = f64(a) + f64(b)
    B = U * ref.abs()
    return ref, with_store16(ref, B), B


def row_stats(ref, B):
    """{sum, sum^2} [rows, 2] over the fp16-rounded rows of ref [rows, H] whose fp32 values are known to within B, and their bounds (docstring)"""
    H = ref.shape[-1]
    xr, d = round16(ref), round16(ref + B) - round16(ref - B)
    a = xr.abs() + d
    st = torch.stack([xr.sum(-1), (xr * xr).sum(-1)], -1)
    E = torch.stack([SECOND * H * U * a.sum(-1) + d.sum(-1), SECOND * (H + 1) * U * (a * a).sum(-1) + (d * (2 * xr.abs() + d)).sum(-1)], -1)
    return st, E


def clip_embed(ids, tok, embeds, pos, rows, T, vocab):
    """-> x (ref, bound), stats (ref, bound)"""
    a = f64(embeds)[:rows] if embeds is not None else f64(tok)[torch.as_tensor(ids).cpu().long().clamp(0, vocab - 1)[:rows]]
    b = f64(pos)[torch.arange(rows) % T]
    ref, bound, B = add16(a, b)
    return (ref, bound), row_stats(ref, B)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------------------
def layer_norm(x, g, b, eps, E=None):
    """fp32 two-pass LayerNorm over the last axis of x (entries already off by E) -> (y, fp32 bound)"""
    x, g, b = f64(x), f64(g), f64(b)
    H = x.shape[-1]
    E = torch.zeros_like(x) if E is None else E
    eps = float(np.float32(eps))
    mean = x.mean(-1, keepdim=True)
    dm = U * x.abs().sum(-1, keepdim=True) + U * mean.abs() + E.mean(-1, keepdim=True)
    d = x - mean
    e = U * d.abs() + dm + E
    var = (d * d).mean(-1, keepdim=True)
    dv = (2 * d.abs() * e + e * e).sum(-1, keepdim=True) / H + (H + 2) * U * var
    w = var + eps
    assert bool((dv < 0.5 * w).all()), "LayerNorm bound: the variance is not resolved"
    rstd = w ** -0.5
    r = (1 - dv / w) ** -0.5 - 1 + 3 * U
    y = d * rstd * g + b
    return y, SECOND * (g.abs() * rstd * (e + d.abs() * (r + 2 * U)) + U * y.abs())


def clip_pool_positions(ids, eos_id):
    """the pooled position of each sequence: eos_id == 2 the first position of the largest id, else the first occurrence of eos_id, 0 when it is absent"""
    ids = torch.as_tensor(ids).cpu().long()
    key = ids if eos_id == 2 else (ids == eos_id).long()
    T = ids.shape[1]
    best = key.max(1, keepdim=True).values
    return torch.where(key == best, torch.arange(T)[None, :], torch.full_like(ids, T)).min(1).values


def clip_pool(ids, x, g, b, eos_id, eps):
    """x [B, T, H] -> (ref [B, H], bound, positions)"""
    p = clip_pool_positions(ids, eos_id)
    rows = f64(x)[torch.arange(len(p)), p]
    y, B = layer_norm(rows, g, b, eps)
    return y, with_store16(y, B), p


def vit_embed(patches, cls, pos, sg, sb, pg, pb, eps, B, T):
    """patches [B (T - 1), H] -> x (ref [B T, H], bound), stats (ref, bound)"""
    H = f64(cls).numel()
    v = torch.cat([f64(cls).reshape(1, 1, H).expand(B, 1, H), f64(patches).reshape(B, T - 1, H)], 1).clone()
    E = torch.zeros_like(v)
    if sg is not None:
        v[:, 1:], E[:, 1:] = layer_norm(v[:, 1:], sg, sb, eps)
    v = v + f64(pos).reshape(1, T, H)
    E = E + U * v.abs()
    if pg is not None:
        v, E = layer_norm(v, pg, pb, eps, E)
    v, E = v.reshape(B * T, H), E.reshape(B * T, H)
    return (v, with_store16(v, E)), row_stats(v, E)


# ---- fp32 dot products -------------------------------------------------------------------------------------------------------------------------------------
def vit_project(X, W):
    """out fp32 [B, N] = X . W^T: K u sum |x w|"""
    X, W = f64(X), f64(W)
    return X @ W.t(), SECOND * X.shape[1] * U * (X.abs() @ W.abs().t())


def hyper_dot(hyper, up):
    """hyper [n, C], up [n, P, C] -> mask fp32 [n, P]: a chain of C FMAs"""
    h, u = f64(hyper), f64(up)
    return torch.einsum("nc,npc->np", h, u), SECOND * h.shape[1] * U * torch.einsum("nc,npc->np", h.abs(), u.abs())


def conv1x1_nchw(x, w, bias):
    """x [B, Ci, HW], w [Co, Ci], bias [Co] -> y [B, Co, HW]: bias and Ci exact products, Ci additions, the fp16 store"""
    x, w, bias = f64(x), f64(w), f64(bias)
    y = torch.einsum("oc,bcp->bop", w, x) + bias[None, :, None]
    B = SECOND * (w.shape[1] + 1) * U * (torch.einsum("oc,bcp->bop", w.abs(), x.abs()) + bias.abs()[None, :, None])
    return y, with_store16(y, B)


# ---- data movement -----------------------------------------------------------------------------------------------------------------------------------------
def patch_gather(px, ps, stride, gh, gw, Kpad):
    """px [B, C, Hi, Wi] -> cols [B gh gw, Kpad], written index by index"""
    B, C = px.shape[:2]
    out = torch.zeros(B, gh, gw, Kpad, dtype=px.dtype)
    for py in range(gh):
        for qx in range(gw):
            out[:, py, qx, :C * ps * ps] = px[:, :, py * stride:py * stride + ps, qx * stride:qx * stride + ps].reshape(B, -1)
    return out.reshape(B * gh * gw, Kpad)


def pixel_shuffle2(g, B, Hs, Ws, Co):
    """g [B Hs Ws, 4 Co], columns (ky, kx, co) -> y [B, 2 Hs, 2 Ws, Co]"""
    return g.reshape(B, Hs, Ws, 2, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hs, 2 * Ws, Co)


# ---- the kernels with a native exponential ---------------------------------------------------------------------------------------------------------------
def _exp_model(x):
    return (x.abs() + 4) * 2.0 ** -23


def _check_share(Xpart, total, what):
    share = float((Xpart / total).max())
    assert share <= 0.1, f"{what}: the modelled exponential takes {share:.3f} of the bound (must stay below a tenth)"
    return share


def causal_attention(qkv, B, T, heads):
    """qkv fp16 [B T, 3 heads 64] -> (out [B T, heads 64], bound, exp_share). q / 8 and the 64 products of a score are exact, its 63 additions give 64 u sum
    |q k| / 8; s - m rounds once. Weight j carries D_j + X_j + sum_i p_i (D_i + X_i) + 12 u (the sum of the exponentials over 2 per lane and 6 butterfly levels,
    the reciprocal, the product), the P.V chain of nk = q + 1 FMAs nk u, then the fp16 store."""
    x = f64(qkv).reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]                                   # [B, h, T, 64]
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
    s = (q @ k.transpose(-1, -2)) / 8
    sa = (q.abs() @ k.abs().transpose(-1, -2)) / 8
    m = s.masked_fill(~vis, -math.inf).max(-1, keepdim=True).values
    xs = torch.where(vis, s - m, torch.zeros_like(s))
    p = torch.softmax(s.masked_fill(~vis, -math.inf), -1)
    D, X = 64 * U * sa + U * xs.abs(), _exp_model(xs)
    nk = torch.arange(1, T + 1, dtype=torch.float64).reshape(T, 1)
    rel = D + X + (p * (D + X)).sum(-1, keepdim=True) + (nk + 12) * U
    out = p @ v
    Bf = SECOND * ((p * rel) @ v.abs())
    Xp = (p * (X + (p * X).sum(-1, keepdim=True))) @ v.abs()
    total = with_store16(out, Bf)
    share = _check_share(Xp, total, "causal_attention")
    fold = lambda t: t.permute(0, 2, 1, 3).reshape(B * T, heads * 64)      # noqa: E731
    return fold(out), fold(total), share


def softmax_rows(x, n, scale):
    """x fp16 [rows, ld] -> (softmax(scale x[:, :n]), bound, exp_share). The argument of exp2 is fma(v, sl, -fl(mx sl)), sl = fl(scale log2 e): the rounding of
    mx sl shifts every argument alike and cancels; sl's two roundings and the FMA's give 3 u |x_j|. The sum of n positive terms in any order n u, the
    reciprocal and the product 3 u, then the fp16 store."""
    v = f64(x)[:, :n]
    xs = (v - v.max(-1, keepdim=True).values) * float(np.float32(scale))
    p = torch.softmax(xs, -1)
    D, X = 3 * U * xs.abs(), _exp_model(xs)
    rel = D + X + (p * (D + X)).sum(-1, keepdim=True) + (n + 3) * U
    Bf = SECOND * p * rel
    total = with_store16(p, Bf)
    return p, total, _check_share(p * (X + (p * X).sum(-1, keepdim=True)), total, "softmax_rows")


def ip_attn_map(Q, Kip, heads):
    """Q fp16 [B, Nq, ldq], Kip fp16 [B, ntok, ldk] -> (attn_map [B, heads, Nq, ntok], bound, exp_share): S[d, t] = softmax over the TOKENS of K_ip[t, d] (v - mx
    rounds once, the sum of at most 16 terms, the reciprocal and the product: 19 u), then a chain of 64 FMAs per output and the fp16 store."""
    B, Nq = Q.shape[:2]
    ntok = Kip.shape[1]
    q = f64(Q)[..., :heads * 64].reshape(B, Nq, heads, 64).permute(0, 2, 1, 3)               # [B, h, Nq, 64]
    kk = f64(Kip)[..., :heads * 64].reshape(B, ntok, heads, 64).permute(0, 2, 3, 1)          # [B, h, 64, ntok]
    xs = kk - kk.max(-1, keepdim=True).values
    S = torch.softmax(xs, -1)
    D, X = U * xs.abs(), _exp_model(xs)
    rel = D + X + (S * (D + X)).sum(-1, keepdim=True) + 19 * U
    out = q @ S
    Bf = SECOND * (q.abs() @ (S * rel) + 64 * U * (q.abs() @ S))
    total = with_store16(out, Bf)
    return out, total, _check_share(q.abs() @ (S * (X + (S * X).sum(-1, keepdim=True))), total, "ip_attn_map")


# the inputs of the GPU cases (built on the CPU, so that test_encoder_ops_cpu.py can check the tenth-of-the-bound condition for every one of them)
ATTN_T = (1, 2, 63, 64, 65, 77, 127, 128)
ATTN_HEADS = (1, 3)
ATTN_EDGES = (0, 63, 64, "q-1", "q")


def _code(idx):
    """+-1 code of an index < 128: its 7 bits, 9 times (63 dims, one zero) -- two different indices agree in at most 63 - 18 places"""
    bits = ((torch.as_tensor(idx).reshape(-1, 1) >> torch.arange(7)) & 1).double() * 2 - 1
    return torch.cat([bits.repeat(1, 9), torch.zeros(len(bits), 1, dtype=torch.float64)], 1)


def attention_case(family, T, heads, seed, edge=None):
    """qkv fp16 [2 T, 3 heads 64]. V = 1 + randn / 4 everywhere (no cancellation in an output, so the half ulp of the store is of the size of the output).
    diffuse: q, k ~ N(0, 1).
    planted: one key per row leads by 20 or more. edge 0 / 63 / 64: that key's row is 2 (1 ...), every query 1.25 (1 ...) (score 20), the other keys N(0, 0.05^2);
             edge q / q-1: query i = 2 code(i), key j = 4.4453 code(j) (or code(j + 1)): score 70 where the codes match, at most 50 elsewhere.
    late:    keys 0 .. 63 score about -60, keys 64 .. about +60 (q = 1 + noise, k = -+7.5 + noise): rows 64 .. find their maximum in the second key half, 120 above
             the first."""
    B, g = 2, gen(seed)
    q, k = torch.randn(B, T, heads, 64, generator=g, dtype=torch.float64), torch.randn(B, T, heads, 64, generator=g, dtype=torch.float64)
    v = 1 + 0.25 * torch.randn(B, T, heads, 64, generator=g, dtype=torch.float64)
    if family == "planted" and edge in (0, 63, 64):
        k = 0.05 * k
        if edge < T:
            k[:, edge] = 2.0
        q = torch.full_like(q, 1.25)
    elif family == "planted":
        idx = torch.arange(T)
        q = (2.0 * _code(idx)).reshape(1, T, 1, 64).expand(B, T, heads, 64)
        k = (4.4453 * _code(idx + (1 if edge == "q-1" else 0))).reshape(1, T, 1, 64).expand(B, T, heads, 64)
    elif family == "late":
        sign = torch.where(torch.arange(T) < 64, -1.0, 1.0).double().reshape(1, T, 1, 1)
        q, k = 1 + 0.05 * q, 7.5 * sign + 0.5 * k
    return torch.stack([q, k, v], 2).reshape(B * T, 3 * heads * 64).half()


def planted_target(T, edge):
    """the dominant key of every query row (-1: none visible)"""
    i = torch.arange(T)
    t = i if edge == "q" else i - 1 if edge == "q-1" else torch.full((T,), edge)
    return torch.where((t <= i) & (t >= 0), t, torch.full((T,), -1))


def attention_cases():
    for T in ATTN_T:
        for heads in ATTN_HEADS:
            yield ("diffuse", T, heads, None)
            for edge in ATTN_EDGES:
                yield ("planted", T, heads, edge)
            if T > 64:
                yield ("late", T, heads, None)


SOFTMAX_N = (8, 2040, 2048, 2056, 4096, 4104, 8192, 8200, 16384)


def softmax_edges(n):
    """the indices on both sides of every 2048 boundary inside a row of n (the middle of a row that has none)"""
    return [e for b in range(2048, n, 2048) for e in (b - 1, b)] or [n // 2]


def softmax_case(family, n, ld, seed, at=None):
    """3 rows fp16 [3, ld] (the gap columns hold 7.0). diffuse: 2 randn; planted: one score 30 above the rest (randn / 4), at index 0, n - 1 and `at` (rows 0, 1,
    2); extreme: values +-60000 less a few fp16 steps (32)"""
    g = gen(seed)
    x = torch.full((3, ld), 7.0, dtype=torch.float64)
    if family == "diffuse":
        x[:, :n] = 2 * torch.randn(3, n, generator=g, dtype=torch.float64)
    elif family == "planted":
        x[:, :n] = 0.25 * torch.randn(3, n, generator=g, dtype=torch.float64)
        for r, i in enumerate([0, n - 1, at]):
            x[r, i] += 30
    else:
        x[:, :n] = torch.where(torch.rand(3, n, generator=g) < 0.5, -60000.0, 60000.0).double() - 32.0 * torch.randint(0, 3, (3, n), generator=g)
    return x.half()


def softmax_cases(n):
    """(family, ld, scale, at) of a row length"""
    for ld in (n, n + 24):
        for scale in (1.0, 0.125):
            yield ("diffuse", ld, scale, None)
            for at in softmax_edges(n):
                yield ("planted", ld, scale, at)
    if n == 2056:
        yield ("extreme", n + 24, 1.0, None)


IPMAP_NTOK, IPMAP_NQ, IPMAP_HEADS = (1, 4, 16), (1, 255, 256, 257), (1, 3)


def ip_map_case(family, ntok, Nq, heads, seed):
    """Q fp16 [2, Nq, heads 64 + 16] = 1 + randn / 4 (positive: no cancellation), K_ip fp16 [2, ntok, heads 64 + 8]: diffuse randn, or planted: per column d one
    token leads by 20 (the token softmax is one-hot)"""
    g = gen(seed)
    Q = 1 + 0.25 * torch.randn(2, Nq, heads * 64 + 16, generator=g, dtype=torch.float64)
    K = torch.randn(2, ntok, heads * 64 + 8, generator=g, dtype=torch.float64)
    if family == "planted":
        lead = torch.randint(0, ntok, (2, 1, heads * 64 + 8), generator=g)
        K = 0.25 * K + 20.0 * (torch.arange(ntok).reshape(1, ntok, 1) == lead).double()
    return Q.half(), K.half()


def ip_map_cases():
    for ntok in IPMAP_NTOK:
        for Nq in IPMAP_NQ:
            for heads in IPMAP_HEADS:
                for family in ("diffuse", "planted"):
                    yield (family, ntok, Nq, heads)


# ---- activations -------------------------------------------------------------------------------------------------------------------------------------------
def erf_poly32(z):
    """erf_as_f of csrc/common.h restated in numpy fp32 (separate roundings where the kernel fuses; a true division and numpy's exp where it takes the hardware's)"""
    z = np.asarray(z, dtype=np.float32)
    f = np.float32
    ax = np.abs(z)
    t = f(1) / (f(0.3275911) * ax + f(1))
    poly = t * (t * (t * (t * (t * f(1.061405429) + f(-1.453152027)) + f(1.421413741)) + f(-0.284496736)) + f(0.254829592))
    r = f(1) - poly * np.exp(-ax * ax)
    assert r.dtype == np.float32
    return np.copysign(r, z)


def all_fp16(lo, hi):
    """every fp16 value in [lo, hi], both zeros included"""
    v = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.float16)
    return v[torch.isfinite(v) & (v >= lo) & (v <= hi)].contiguous()


def gelu_erf_cpu_error():
    """the largest |erf_poly32 - erf| over z = fl(x / sqrt 2), x every fp16 value in [-8, 8]"""
    z = all_fp16(-8, 8).float().numpy() * np.float32(0.70710678118654752440)
    return float(np.abs(erf_poly32(z).astype(np.float64) - torch.special.erf(torch.from_numpy(z.astype(np.float64))).numpy()).max())


def gelu(x):
    """exact GELU of fp16 x: 0.5 x erfc(-x / sqrt 2) in fp64 (no cancellation in the negative tail), and the bound of the docstring"""
    x = f64(x)
    y = 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    B = SECOND * (0.5 * x.abs() * (GELU_ERF_CPU + 11 * U) + 4 * U * y.abs())
    return y, with_store16(y, B)


# ---- the UNet's embeddings ---------------------------------------------------------------------------------------------------------------------------------
def sinusoid(val, width):
    """val fp64 [...] -> [..., width] = [cos(val f_k) | sin(val f_k)], k < width / 2, and the fp32 bound of the docstring"""
    half = width // 2
    y = LN1E4 * torch.arange(half, dtype=torch.float64) / half
    a = f64(val).unsqueeze(-1) * torch.exp(-y)
    da = a.abs() * (3 * U * y + 5 * U)
    return torch.cat([torch.cos(a), torch.sin(a)], -1), SECOND * torch.cat([da, da], -1) + 2.0 ** -22


def sinusoid_diffusers(val, width):
    """diffusers `get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0)` restated with torch in fp32"""
    half = width // 2
    exponent = -math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / (half - 0.0)
    emb = torch.as_tensor(val).float().reshape(-1, 1) * torch.exp(exponent)[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
    return torch.cat([emb[:, half:], emb[:, :half]], dim=-1)


def embed(ts, text_embeds, time_ids, Tp, Ad):
    """ts fp32 [B], text_embeds fp16 [B, P] or None, time_ids fp16 [B, nids] -> tsin (ref, fp32 bound), addin (ref, fp32 bound) (the text columns: bound 0)"""
    tsin = sinusoid(f64(ts), Tp)
    B = len(ts)
    ids, idb = sinusoid(f64(time_ids), Ad)
    parts = ([f64(text_embeds)] if text_embeds is not None else []) + [ids.reshape(B, -1)]
    bounds = ([torch.zeros_like(f64(text_embeds))] if text_embeds is not None else []) + [idb.reshape(B, -1)]
    return tsin, (torch.cat(parts, 1), torch.cat(bounds, 1))
