"""fp64 references of the UNet's own launches -- the GEMM with its plain / K-split / GEGLU / folded-LayerNorm epilogues, the 3x3 and boundary convolutions, GroupNorm(+SiLU)
and LayerNorm, the element-wise sampler steps and the skinny linear -- and next to each the error bound its HIP kernel must meet (None: the exact bits). Written in the
manner of llm_ops_ref.py / encoder_ops_ref.py / attn_ops_ref.py, whose notation it keeps: u = 2^-24, SECOND covers second-order terms.

The MFMA k-loop is NOT modelled: its error is taken out of the budget by the inputs. Every bound below is derived from the operations read in the kernel source
(csrc/gemm_epilogue.h, common.h, norm.hip, gn_fold.h, misc.hip), never from what a kernel returned.

  lattice       operands are integers in [-3, 3] times a power of two (fp16 values). A product of two of them is exact in fp32; every partial sum, in any order, is an
                integer multiple of the product of the two units and stays below 2^24 of them (`exactness(case)`, asserted for every case in test_unet_ops_cpu.py):
                an fp32 accumulation is EXACT whatever an MFMA does inside and however K is split over stages, waves, slabs and workgroups.
  plain epilogue  h = fp16(acc + bias); out = fp16(h + rowvec + residual) (gemm_epilogue.h: the layer's output is an fp16 tensor before the time-embedding row or the
                residual is added). acc + bias and h + rowvec + residual are lattice sums below 2^24 units: exact in fp32. What is left are the two fp16 roundings: the
                reference applies them (round16) and the kernel must give its bits. Bias, time-embedding row and residual are chosen so that some outputs need rounding
                at both points and some at neither; conv_in / conv_out / linear_small round once.
  GEGLU         value and gate h are exact fp16 lattice values; out = fp16(fl(v fl(g P))), P = fma(f - floor f, e.y, e.x), f = fma(clamp(g, -8, 7.99), 32, 256) (common.h
                gelu_lut_f; the table {Phi(x_i), Phi(x_i+1) - Phi(x_i)}, x_i = (i - 256) / 32, is built in double and rounded to fp32, gemm.hip). Against v g Phi(g):
                  interpolation  h^2 / 8 max |Phi''| over the gate's own cell, h = 1 / 32; Phi''(x) = -x phi(x) is monotonic between 0 and +-1, which are cell borders,
                                 so the maximum lies at a border of the cell
                  clamp          |Phi(clamp g) - Phi(g)| (below 7e-16)
                  table, FMAs    u Phi(x_i) + u (Phi(x_i+1) - Phi(x_i)) (the two entries), 512 u * 0.39895 / 32 (f rounds at a magnitude below 512; the interpolant's slope
                                 per unit of f is at most phi(0) / 32), u (the final FMA, a value of at most 1)
                then the two products, 2 u |ref|, and the fp16 store.
  GroupNorm     statistics on a lattice (x a multiple of 1/4, |x| <= 6: sum x and sum x^2 are sums of integers times 2^-4 below 2^24 of them): the fp32 partial sums of all
                three kernels are exact, the fold from there on is fp64. mean and 1 / sqrt(var + eps) are rounded to fp32 (u each); sc = fl(rstd gamma) (2 u in all), used
                for the shift too, so that its error scales x - mean: |x - mean| |sc| 2 u; the rounding of mean moves the output by u |mean| |sc|; sh = beta - mean sc and
                x sc + sh, contracted into FMAs or not: u (|mean sc| + |sh|) + u (|x sc| + |y|). For real inputs the fp32 partial sums of the kernel's own reduction tree are
                added (`gn_depth`): a value passes through at most d additions, d u sum |x| and d u sum x^2, which reach the variance amplified by mean^2 / var.
  SiLU          y / (1 + exp(-y)): the error E of y passes through |silu'| <= 1.1; the native exponential is MODELLED (`_exp_model`, the only model in this file) as off by
                X = (|y| + 4) 2^-23 relatively, which reaches the result as (1 - s) X, s = sigmoid(y); 1 + e, the 1-ulp v_rcp_f32 (2 u) and the product: 4 u. Every SiLU case
                must keep the model's share of its bound below a tenth (the share is the third value `gn_ref` and `linear_ref` return).
  LayerNorm     two passes in fp32 (norm.hip layernorm_kernel): encoder_ops_ref's derivation, with the sum of the row exact on the lattice and the sum of squares
                counted from the kernel's reduction tree (`ln_ref`).
  folded LayerNorm  common.h ln_mean_rstd_f / ln_fold_f on exact {sum, sum of squares} and an exact accumulator: mean = fl(s1 / K) (u |mean|); var = fma(s2, 1 / K,
                -fl(mean^2)): 3 u mean^2 + u var (+ u s2 / K where 1 / K is not a power of two); rstd: u for the addition of eps, 2 u for rsqrtf; inner = fma(-mean, cs, acc):
                u |mean| |cs| + u |inner| -- the cancellation of acc - mean colsum shows here: |mean cs| may be a hundred times |inner|; out = fma(rstd, inner, lb).
  element-wise  the 3 .. 6 fp32 roundings of each formula, one u per operation on the magnitude it produces, whether or not the compiler contracts a product into the
                addition behind it (a contraction removes a rounding), then the fp16 store (none for prior_step).
"""
import math

import numpy as np
import torch

from llm_ops_ref import SECOND, U, f64, half_ulp16, ratio  # noqa: F401
from encoder_ops_ref import round16, with_store16, _exp_model  # noqa: F401

NTILES = 28
ALL_TILES = tuple([-1] + list(range(NTILES)))
LIMIT = 2.0 ** 24
SQRT2 = math.sqrt(2.0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, g, lo=-3, hi=3):
    """integers in [lo, hi] as fp64"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def f32(v):
    return float(np.float32(v))


# ---- the comparison every GPU test and every mutant goes through ---------------------------------------------------------------------------------------------
def worst(got, ref, bound=None):
    """-> (ok, max(err / bound) or the number of differing elements, index of the worst element). bound None: the exact bits (as values: -0 == 0)"""
    got, ref = f64(got).reshape(ref.shape), f64(ref)
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).reshape(-1).nonzero()[0]
        return False, float("inf"), tuple(int(i) for i in np.unravel_index(int(bad), tuple(ref.shape)))
    err = (got - ref).abs()
    if bound is None:
        r, n = err, float((err != 0).sum())
    else:
        r = torch.where(err == 0, torch.zeros_like(err), err / f64(bound))
        n = float(r.max()) if r.numel() else 0.0
    at = tuple(int(i) for i in np.unravel_index(int(r.reshape(-1).argmax()), tuple(ref.shape))) if r.numel() else ()
    return (n == 0.0 if bound is None else n <= 1.0), n, at


def accept(tag, got, ref, bound=None, axes=None):
    """assert that `got` is `ref` to the bit (bound None) or within `bound` element by element; the message names the worst element. -> max(err / bound) (0 if exact)"""
    ok, n, at = worst(got, ref, bound)
    if not ok:
        g, r = f64(got).reshape(ref.shape)[at], f64(ref)[at]
        where = dict(zip(axes, at)) if axes else at
        what = f"{int(n)} elements differ" if bound is None and math.isfinite(n) else f"max(err / bound) {n:.4g}"
        raise AssertionError(f"{tag}: {what}; worst at {where}: got {float(g)!r}, reference {float(r)!r}" + ("" if bound is None else f", bound {float(f64(bound)[at]):.3g}"))
    return 0.0 if bound is None else n


def scrambled_fp32_sum(terms, seed, chunk=32):
    """sum over the last axis in fp32: chunks of `chunk` terms in a scrambled order, each chunk summed on its own, the chunk sums added in another scrambled order"""
    t = f64(terms).numpy().astype(np.float32)
    K = t.shape[-1]
    rs = np.random.RandomState(seed)
    t = t[..., rs.permutation(K)]
    pad = (-K) % chunk
    if pad:
        t = np.concatenate([t, np.zeros(t.shape[:-1] + (pad,), np.float32)], -1)
    t = t.reshape(t.shape[:-1] + (-1, chunk))
    part = np.zeros(t.shape[:-1], np.float32)
    for i in range(chunk):
        part = (part + t[..., i]).astype(np.float32)
    part = part[..., rs.permutation(part.shape[-1])]
    acc = np.zeros(part.shape[:-1], np.float32)
    for i in range(part.shape[-1]):
        acc = (acc + part[..., i]).astype(np.float32)
    return torch.from_numpy(acc.astype(np.float64))


# ---- GEMM, plain epilogue ------------------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = ((37, 132, 64), (333, 200, 192), (257, 328, 128), (64, 64, 2560))
GEMM_EPILOGUES = ("none", "bias", "residual", "bias+residual", "bias+aliased residual")
SPLITK_SHAPES = ((77, 192, 640, 5), (300, 64, 128, 2), (130, 136, 1152, 3))
SPLITK_TILES = (-1, 0, 4, 8, 12, 18, 19, 20, 21, 22, 23)
WUNIT = 2.0 ** -8          # the weights' lattice unit (activations: 1)


def column_bias(N):
    """fp16 bias, every column its own (up to 384 columns): 48 + (j % 448) / 32 on every third column -- there acc + bias lies in [32, 64), where fp16 steps by 2^-5 and the
    accumulator's 2^-8 bits are rounded away -- and (j % 384) / 64 - 3 on the others, which with acc mostly stay below 4, where every multiple of 2^-8 is an fp16 value"""
    j = torch.arange(N)
    return torch.where(j % 3 == 1, 48.0 + (j % 448).double() * 2.0 ** -5, (j % 384).double() * 2.0 ** -6 - 3.0)


def row_residual(M, N, g):
    """fp16 residual, every row its own level ((i % 13) - 6) / 2, a 2^-8 lattice on top"""
    i = torch.arange(M).reshape(M, 1)
    return ((i % 13) - 6).double() * 0.5 + ints((M, N), g) * WUNIT


def gemm_case(M, N, K, seed=None):
    g = gen(1000 + M + 3 * N + 7 * K if seed is None else seed)
    A, W = ints((M, K), g), ints((N, K), g) * WUNIT
    return dict(M=M, N=N, K=K, A=A.half(), W=W.half(), bias=column_bias(N).half(), res=row_residual(M, N, g).half(), unit=WUNIT)


def gemm_parts(case, bias=True, residual=True):
    """-> acc, h = acc + bias, h16 = fp16(h), s = h16 + residual, out = fp16(s) (fp64 tensors)"""
    acc = f64(case["A"]) @ f64(case["W"]).t()
    h = acc + f64(case["bias"]) if bias else acc
    h16 = round16(h)
    s = h16 + f64(case["res"]) if residual else h16
    return acc, h, h16, s, round16(s)


def gemm_ref(case, epilogue="bias+residual"):
    return gemm_parts(case, "bias" in epilogue, "residual" in epilogue)[4], None


def exactness(case):
    """the largest magnitude any partial sum of any output can reach, whatever the order, in units of the product lattice: sum_k |a_k w_k|, plus |bias|, |time-embedding
    row| and |residual| (the epilogue's fp32 additions). Must stay below 2^24."""
    if "x" in case:
        return conv_exactness(case)
    a = f64(case["A"]).abs() @ f64(case["W"]).abs().t()
    for k in ("bias", "res"):
        if case.get(k) is not None:
            a = a + f64(case[k]).abs()
    return float(a.max()) / case["unit"]


# ---- GEGLU ---------------------------------------------------------------------------------------------------------------------------------------------------
GEGLU_SHAPES = ((130, 8 * 64, 64), (37, 8 * 160, 192), (257, 8 * 80, 128))
GEGLU_TILES = (-1, 0, 2, 4, 8, 10, 12, 18, 19, 20, 21, 22, 27)
GATE_UNIT = {64: 2.0 ** -3, 128: 2.0 ** -4, 192: 2.0 ** -4}


def geglu_case(M, N, K, seed=None):
    """A [M, K] integers; W [N, K]: rows [0, N / 2) the values (unit 2^-6), rows [N / 2, N) the gates (unit 2^-3 / 2^-4: gates of standard deviation about 3.5, with the
    bias beyond +-9); per-column biases. Value and gate sums are fp16 lattice values (asserted on the CPU)."""
    g = gen(2000 + M + N + K if seed is None else seed)
    H = N // 2
    A = ints((M, K), g)
    W = torch.cat([ints((H, K), g) * 2.0 ** -6, ints((H, K), g) * GATE_UNIT[K]])
    j = torch.arange(H)
    bias = torch.cat([(j % 29 - 14).double() * 2.0 ** -3, (j % 37 - 18).double() * 0.25])
    return dict(M=M, N=N, K=K, A=A.half(), W=W.half(), bias=bias.half(), res=None, unit=2.0 ** -6)


def phi(x):
    return 0.5 * torch.special.erfc(-f64(x) / SQRT2)


def _pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def lut_cell(g):
    """the table cell gelu_lut_f reads for a gate (the value of f = clamp(g) 32 + 256 taken exactly) -> (index, clamped gate)"""
    gc = f64(g).clamp(-8.0, f32(7.99))
    return torch.floor(gc * 32.0 + 256.0), gc


def geglu_apply(v, g, Ev=None, Eg=None):
    """out = fp16(v g P(g)) for fp16 v, g that are off from the reference's by at most Ev, Eg (None: exact) -> (ref, bound)"""
    v, g = f64(v), f64(g)
    P = phi(g)
    ref = v * g * P
    i, gc = lut_cell(g)
    x0 = (i - 256.0) / 32.0
    x1 = x0 + 1.0 / 32.0
    interp = (1.0 / 32.0) ** 2 / 8.0 * torch.maximum((x0 * _pdf(x0)).abs(), (x1 * _pdf(x1)).abs())
    if Ev is not None:          # the kernel's gate may lie in a neighbouring cell: max |Phi''| = phi(1) everywhere
        interp = torch.full_like(interp, (1.0 / 32.0) ** 2 / 8.0 * 0.24198)
    clamp = (phi(gc) - P).abs() + 1e-15
    rounding = U * phi(x0) + U * (phi(x1) - phi(x0)) + 512.0 * U * 0.39895 / 32.0 + U
    dP = interp + clamp + SECOND * rounding
    B = (v * g).abs() * dP + SECOND * 2 * U * ref.abs()
    if Ev is not None:
        B = B + SECOND * (Ev * (g * P).abs() + v.abs() * (P + (g * _pdf(g)).abs() + 0.5 * Eg) * Eg + 1.2 * Ev * Eg)      # gelu' = Phi + g phi (|.| <= 1.13); |gelu''| <= 0.8
    return ref, with_store16(ref, B)


def geglu_ref(case):
    h = f64(case["A"]) @ f64(case["W"]).t() + f64(case["bias"])
    H = case["N"] // 2
    return geglu_apply(round16(h[:, :H]), round16(h[:, H:]))


# ---- convolutions ----------------------------------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = ((2, 9, 7, 64, 72, 1, 0), (1, 10, 14, 64, 64, 2, 0), (2, 8, 8, 128, 64, 1, 1), (1, 16, 16, 64, 160, 1, 0), (1, 16, 48, 64, 100, 1, 0))
CONV_ALL_TILES = (CONV_SHAPES[0], CONV_SHAPES[3])
CONV_HALO = (CONV_SHAPES[3], CONV_SHAPES[4])
CONV_CAT_SHAPES = ((2, 9, 7, 128, 64, 192), (1, 16, 16, 64, 128, 96))
CONV_IN_SHAPES = ((2, 4, 13, 9, 64), (1, 7, 5, 5, 8))          # B, Cin, H, W, Co
CONV_OUT_SHAPES = ((2, 128, 13, 9, 3), (2, 64, 5, 7, 1))       # B, C, H, W, Co
CONV_AXES = ("b", "y", "x", "co")


def out_hw(H, W, stride, up):
    H, W = (2 * H, 2 * W) if up else (H, W)
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def conv_case(B, H, W, Cin, Co, stride=1, up=0, seed=None, Cin2=0):
    """x [B, H, W, Cin] integers, w [Co, Cin, 3, 3] on the 2^-8 lattice, bias per output channel, a time-embedding row per image, a residual per pixel (its level
    ((y Wo + x) % 13 - 6) / 2); Cin2: the appended 1x1 shortcut's input x2 [B, H, W, Cin2] and weight wsc [Co, Cin2] (no row, no residual: ia2p_conv3x3_cat)"""
    g = gen(3000 + B + H * 3 + W * 5 + Cin + Co + stride + up + Cin2 if seed is None else seed)
    Ho, Wo = out_hw(H, W, stride, up)
    c = dict(B=B, H=H, W=W, Cin=Cin, Co=Co, stride=stride, up=up, Ho=Ho, Wo=Wo, unit=WUNIT,
             x=ints((B, H, W, Cin), g).half(), w=(ints((Co, Cin, 3, 3), g) * WUNIT).half(), bias=column_bias(Co).half())
    if Cin2:
        c.update(Cin2=Cin2, x2=ints((B, H, W, Cin2), g).half(), wsc=(ints((Co, Cin2), g) * WUNIT).half(), tv=None, res=None)
    else:
        co = torch.arange(Co)
        tv = (torch.arange(B).reshape(B, 1) + 1).double() * 0.5 + (co % 8).double() * 2.0 ** -6 + ints((B, Co), g) * WUNIT
        p = torch.arange(Ho * Wo).reshape(1, Ho, Wo, 1)
        res = ((p % 13) - 6).double() * 0.5 + ints((B, Ho, Wo, Co), g) * WUNIT
        c.update(tv=tv.half(), res=res.half())
    return c


def conv3x3_sum(x, w, stride=1, up=0):
    """x [B, H, W, Ci], w [Co, Ci, 3, 3] fp64 -> [B, Ho, Wo, Co]: nine shifted matrix products over the zero-padded (nearest-upsampled) image"""
    x, w = f64(x), f64(w)
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, Ci = x.shape
    xp = torch.zeros(B, H + 2, W + 2, Ci, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] @ w[:, :, ky, kx].t()
    return out


def conv_exactness(c):
    a = conv3x3_sum(f64(c["x"]).abs(), f64(c["w"]).abs(), c.get("stride", 1), c.get("up", 0))
    if c.get("x2") is not None:
        a = a + f64(c["x2"]).abs() @ f64(c["wsc"]).abs().t()
    a = a + f64(c["bias"]).abs()
    if c.get("tv") is not None:
        a = a + f64(c["tv"]).abs()[:, None, None, :] + f64(c["res"]).abs()
    return float(a.max()) / c["unit"]


def conv_ref(c, drop_tap=None, acc=None):
    """[B, Ho, Wo, Co]: fp16(fp16(conv + bias) + row + residual), or fp16(conv + shortcut + bias) for the appended form. drop_tap = (b, y, x, ky, kx): that tap
    of that output pixel is left out (the mutant of test_unet_ops_cpu.py); acc: the convolution sums, if the caller has them"""
    acc = conv3x3_sum(c["x"], c["w"], c["stride"], c["up"]) if acc is None else acc.clone()
    if drop_tap is not None:
        b, y, x, ky, kx = drop_tap
        assert c["stride"] == 1 and not c["up"]
        yy, xx = y + ky - 1, x + kx - 1
        assert 0 <= yy < c["H"] and 0 <= xx < c["W"]
        acc[b, y, x] -= f64(c["w"])[:, :, ky, kx] @ f64(c["x"])[b, yy, xx]
    if c.get("x2") is not None:
        return round16(acc + f64(c["x2"]) @ f64(c["wsc"]).t() + f64(c["bias"])), None
    h16 = round16(acc + f64(c["bias"]))
    if c.get("tv") is None:
        return h16, None
    return round16(h16 + f64(c["tv"])[:, None, None, :] + f64(c["res"])), None


def boundary_case(kind, B, Ci, H, W, Co, seed=None):
    """conv_in: x NCHW [B, Ci, H, W]; conv_out: x channels-last [B, H, W, Ci]; w [Co, Ci, 3, 3] on the 2^-6 lattice, a bias per output channel"""
    g = gen(4000 + B + Ci + 3 * H + 5 * W + Co if seed is None else seed)
    x = ints((B, H, W, Ci), g)
    w = ints((Co, Ci, 3, 3), g) * 2.0 ** -6
    bias = (torch.arange(Co) % 16 - 8).double() * 2.0 ** -4 + 24.0 * (torch.arange(Co) % 2)
    return dict(kind=kind, B=B, H=H, W=W, Cin=Ci, Co=Co, stride=1, up=0, unit=2.0 ** -6, x=x.half(), w=w.half(), bias=bias.half(), tv=None, res=None)


def boundary_ref(c):
    """-> [B, H, W, Co] = fp16(conv + bias): one rounding (misc.hip conv_in_kernel / conv_out_kernel)"""
    return round16(conv3x3_sum(c["x"], c["w"]) + f64(c["bias"])), None


# ---- GroupNorm (+ SiLU) ----------------------------------------------------------------------------------------------------------------------------------------
GN_GROUPS = 32
# (B, HW, C): the single-pass kernel's three chunk counts at Cg = 10, 20, 30, 40, 60, 80 (HW = 64 or the ragged 70); its deeper instantiations <5, 6> and <10, 16>; the
# two-pass kernels where the single pass refuses (Cg = 4: a chunk would span three groups; 80 chunks of 320 pixels on 32 workgroups: too slow a fill), V = 1 and 2
GN_SHAPES = ((2, 64, 320), (1, 70, 640), (2, 70, 960), (1, 64, 1280), (1, 70, 1920), (2, 64, 2560), (1, 400, 320), (1, 300, 2560), (2, 70, 128), (1, 320, 2560))
GN_VARIANTS = ((1, 1e-5), (0, 1e-5), (1, 1e-6), (0, 1e-6))          # (silu, eps)
GN_REAL_SHAPES = ((2, 64, 320), (2, 70, 128))


def gn_route(B, HW, C, G=GN_GROUPS):
    """the dispatch of ia2p_launch_groupnorm (norm.hip gn_fused_launch) restated -> ("fused", NCH, IT) or ("twopass", V). The GPU tests can observe only which of the
    two families ran (the two-pass kernels write the caller's `partial`); NCH, IT and V are this restatement's word and must follow gn_fused_launch when its
    thresholds change"""
    Cg = C // G
    nvec = C // 8
    V = 1
    while nvec // V > 256 or nvec % V:
        V += 1
    two = ("twopass", V)
    if C % G or C % 8 or Cg < 8:
        return two
    gs = 1
    while (gs * Cg) % 8:
        gs += 1
    nch = gs * Cg // 8
    if G % gs or nch not in (5, 10, 15) or gs > 16:
        return two
    P = 192 if nch == 5 else 64
    it = (HW + P - 1) // P
    if (G // gs) * B < 200 and HW * nch * 16 > 48 * 1024:
        return two
    for cap in {5: (2, 6, 22), 10: (4, 16), 15: (4, 16)}[nch]:
        if it <= cap:
            return ("fused", nch, cap)
    return two


def gn_chunks(B, HW):
    chunks = 1
    while chunks < 64 and B * chunks < 512 and HW // (chunks * 2) >= 8:
        chunks *= 2
    rows = (HW + chunks - 1) // chunks
    return (HW + rows - 1) // rows, rows


def gn_depth(B, HW, C, G=GN_GROUPS):
    """the largest number of fp32 additions a value passes through in the statistics of the kernel gn_route names (read from norm.hip), before the fold goes on in fp64"""
    route = gn_route(B, HW, C, G)
    if route[0] == "fused":
        P = 192 if route[1] == 5 else 64
        return 8 * ((HW + P - 1) // P) + 6                          # a lane's 8 elements of each of its pixels, one after the other; six butterfly levels
    V = route[1]
    TX = C // 8 // V
    TY = 256 // TX
    chunks, rows = gn_chunks(B, HW)
    nsl = 256 // G
    return (rows + TY - 1) // TY + 1 + TY + C // G + (chunks + nsl - 1) // nsl      # a thread's rows (+ 1: the square, not contracted), the row slices, the group's channels, the chunks


def gn_case(B, HW, C, seed=None, real=False):
    """x [B, HW, C] fp16. Lattice: group g of image b has mean ((g + 3 b) % 7) - 3 and spread 1 + g % 3, x = mean + spread t, t in {-1, -3/4, .., 1}. real: 2 randn + 0.7
    and +40 on the first group (E[x^2] - mean^2 would lose the variance there). gamma = 1/2 + (c % 16) / 16, beta = ((c % 11) - 5) / 8"""
    g = gen(5000 + B + HW + C if seed is None else seed)
    Cg = C // GN_GROUPS
    grp = torch.arange(C) // Cg
    if real:
        x = 2.0 * torch.randn(B, HW, C, generator=g, dtype=torch.float64) + 0.7
        x[:, :, :Cg] += 40.0
    else:
        b = torch.arange(B).reshape(B, 1, 1)
        x = (((grp + 3 * b) % 7) - 3).double() + (1 + grp % 3).double() * ints((B, HW, C), g, -4, 4) * 0.25
    c = torch.arange(C)
    return dict(B=B, HW=HW, C=C, real=real, x=x.half(), gamma=(0.5 + (c % 16).double() / 16).half(), beta=(((c % 11) - 5).double() / 8).half())


def gn_stats(case, shift_channel=None):
    """{sum x, sum x^2} per (image, group) in fp64 [B, G, 2]. shift_channel = (g, +-1): the mutant -- group g's first (-1: it goes to g - 1) or last (+1: to g + 1)
    channel is counted into the neighbouring group"""
    x = f64(case["x"])
    B, HW, C = x.shape
    Cg = C // GN_GROUPS
    grp = torch.arange(C) // Cg
    if shift_channel is not None:
        gq, d = shift_channel
        grp = grp.clone()
        grp[gq * Cg if d < 0 else (gq + 1) * Cg - 1] = gq + d
    onehot = (grp.reshape(C, 1) == torch.arange(GN_GROUPS).reshape(1, -1)).double()
    return torch.stack([x.sum(1) @ onehot, (x * x).sum(1) @ onehot], -1)


def stats_exactness(case):
    """the statistics sums of a lattice case in the units they are multiples of (sum |x| in 1/4, sum x^2 in 1/16): must stay below 2^24"""
    x = f64(case["x"])
    assert bool((x * 4 == torch.floor(x * 4)).all())
    if x.dim() == 3:
        B, HW, C = x.shape
        x = x.reshape(B, HW, GN_GROUPS, C // GN_GROUPS).permute(0, 2, 1, 3).reshape(B * GN_GROUPS, -1)
    return max(float(x.abs().sum(-1).max()) * 4, float((x * x).sum(-1).max()) * 16)


def silu_bound(y, E):
    """y / (1 + exp(-y)) of a y known to within E -> (silu(y), fp32 bound, the modelled exponential's part of it)"""
    s = torch.sigmoid(y)
    out = y * s
    X = out.abs() * (1 - s) * _exp_model(y)
    return out, SECOND * ((s * (1 + y * (1 - s))).abs() * E + X + 4 * U * out.abs() + 0.55 * E * E), X


def gn_ref(case, silu, eps, stats=None):
    """-> (ref [B, HW, C], bound, share of the modelled exponential in the bound (0 without SiLU))"""
    x, gamma, beta = f64(case["x"]), f64(case["gamma"]), f64(case["beta"])
    B, HW, C = x.shape
    Cg = C // GN_GROUPS
    n = float(HW * Cg)
    st = gn_stats(case) if stats is None else stats
    xg = x.reshape(B, HW, GN_GROUPS, Cg)
    if case["real"]:
        d = gn_depth(B, HW, C)
        da, dq = d * U * xg.abs().sum((1, 3)), d * U * (xg * xg).sum((1, 3))
    else:
        da = dq = torch.zeros(B, GN_GROUPS, dtype=torch.float64)
    mean, q = st[..., 0] / n, st[..., 1] / n
    var = (q - mean * mean).clamp_min(0)
    w = var + f32(eps)
    dm = da / n
    dv = dq / n + 2 * mean.abs() * dm + dm * dm + 2.0 ** -50 * q
    assert bool((dv < 0.5 * w).all()), "GroupNorm bound: the variance is not resolved"
    rstd = w ** -0.5
    r = (1 - dv / w) ** -0.5 - 1 + U
    ex = lambda t: t.reshape(B, 1, GN_GROUPS, 1)      # noqa: E731
    sc = ex(rstd) * gamma.reshape(1, 1, GN_GROUPS, Cg)
    sh = beta.reshape(1, 1, GN_GROUPS, Cg) - ex(mean) * sc
    y = xg * sc + sh
    E = SECOND * ((xg - ex(mean)).abs() * sc.abs() * (ex(r) + 2 * U) + (ex(dm) + U * ex(mean).abs()) * sc.abs() + U * ((ex(mean) * sc).abs() + sh.abs() + (xg * sc).abs() + y.abs()))
    y, E = y.reshape(B, HW, C), E.reshape(B, HW, C)
    if not silu:
        return y, with_store16(y, E), 0.0
    out, Bf, X = silu_bound(y, E)
    total = with_store16(out, Bf)
    return out, total, float((X / total).max())


# ---- GroupNorm from producer-side column sums (gn_fold.h) ------------------------------------------------------------------------------------------------------
GN_STATS_SHAPES = ((3, 64, 64, 64, 64, 0), (2, 256, 192, 128, 128, 256))          # B, HW, C, C0 (the first source's channels), slot rows of source 0 and of source 1
GEMM_GNSTATS_SHAPES = ((512, 320, 64, 256), (512, 320, 128, 256))                 # M, N, K, HW: test_gn_fused_gpu.py's smallest, and two k-tiles of it (a K split)
CONV_GNSTATS_SHAPES = ((1, 16, 16, 64, 160), (3, 16, 48, 128, 96))                # B, H, W, Cin, Co of ia2p_conv3x3_gn's producer form: whole 16 x 16 patches


def colstats_ref(x2d, rows):
    """{sum, sum of squares} per slot of `rows` rows and per column, fp64 [M / rows, C, 2] (norm.hip gn_colstats_kernel: fp32 over aligned runs of 16 rows, fp64 from
    there on -- exact where colstats_exactness stays below 2^24)"""
    x = f64(x2d)
    M, C = x.shape
    xs = x.reshape(M // rows, rows, C)
    return torch.stack([xs.sum(1), (xs * xs).sum(1)], -1)


def colstats_exactness(x2d, unit):
    """the largest fp32 partial sum of a run of 16 rows, in the units the sums are multiples of (unit for the values, unit^2 for the squares)"""
    x = f64(x2d)
    assert bool((x / unit == torch.floor(x / unit)).all())
    xs = x.reshape(x.shape[0] // 16, 16, -1)
    return max(float(xs.abs().sum(1).max()) / unit, float((xs * xs).sum(1).max()) / unit ** 2)


def gemm_gnstats_case(M, N, K, HW):
    """a lattice GEMM whose stored outputs stay below 4 (bias (j % 64) / 32 - 1, no residual): multiples of 2^-8 whose squares add exactly over 16 rows"""
    c = gemm_case(M, N, K)
    c.update(bias=((torch.arange(N) % 64).double() / 32 - 1).half(), res=None, HW=HW)
    return c


def conv_gnstats_case(B, H, W, Cin, Co):
    """the same for a 3x3 convolution (ia2p_conv3x3_gn without input statistics: a plain convolution that leaves the column sums of its output): no time-embedding
    row, no residual, out = fp16(conv + bias) below 4"""
    c = conv_case(B, H, W, Cin, Co)
    c.update(bias=((torch.arange(Co) % 64).double() / 32 - 1).half(), tv=None, res=None)
    return c


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = ((77, 128), (5, 2048), (6, 640), (7, 1280))          # one per instantiation (1 .. 4 vectors of 8 per lane); M = 5: a ragged last workgroup


def ln_case(M, C, seed=None):
    """x [M, C]: row i has mean (i % 7) - 3 and spread 1 + i % 3 on the 1/4 lattice; gamma, beta as in gn_case"""
    g = gen(6000 + M + C if seed is None else seed)
    i = torch.arange(M).reshape(M, 1)
    x = ((i % 7) - 3).double() + (1 + i % 3).double() * ints((M, C), g, -4, 4) * 0.25
    c = torch.arange(C)
    return dict(M=M, C=C, x=x.half(), gamma=(0.5 + (c % 16).double() / 16).half(), beta=(((c % 11) - 5).double() / 8).half())


def ln_ref(case, eps):
    """norm.hip layernorm_kernel: mean = fl(sum / C) (the sum is exact on the lattice; the division is charged 2 u, a reciprocal and a product, so that the bound
    does not rest on a correctly rounded division), d = fl(x - mean), var = fl(sum d^2 / C), rstd = rsqrtf(fl(var + eps)), y = fp16(fl(fl(fl(d rstd) gamma) + beta))
    -- encoder_ops_ref.layer_norm's derivation without the summation error of the mean, and with the sum of squares counted from the kernel's own tree: a lane adds
    the 8 elements of each of its NV = ceil(C / 512) vectors one after the other (+ 1 where the square is not contracted into the addition), then six butterfly
    levels; non-negative terms, so 8 NV + 7 roundings are that many u of the sum; the division by C 2 u more"""
    x, g, b = f64(case["x"]), f64(case["gamma"]), f64(case["beta"])
    H = x.shape[-1]
    depth = 8 * ((H // 8 + 63) // 64) + 7
    mean = x.mean(-1, keepdim=True)
    dm = 2 * U * mean.abs()
    d = x - mean
    e = U * d.abs() + dm
    var = (d * d).mean(-1, keepdim=True)
    dv = (2 * d.abs() * e + e * e).sum(-1, keepdim=True) / H + (depth + 2) * U * var
    w = var + f32(eps)
    rstd = w ** -0.5
    r = (1 - dv / w) ** -0.5 - 1 + 3 * U
    y = d * rstd * g + b
    return y, with_store16(y, SECOND * (g.abs() * rstd * (e + d.abs() * (r + 2 * U)) + U * y.abs()))


# ---- element-wise steps ----------------------------------------------------------------------------------------------------------------------------------------
EW_SIZES = ((1, 1, 1), (1, 1, 63), (1, 1, 64), (1, 1, 65), (4, 3, 33 * 33))          # (B, C, HW): n = B C HW, per = C HW


def ew_case(B, C, HW, seed=None):
    g = gen(7000 + B + C + HW if seed is None else seed)
    n = B * C * HW
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    row = torch.arange(B).double()
    return dict(B=B, C=C, HW=HW, n=n, per=C * HW, x=rn(n).half(), eu=rn(n).half(), ec=rn(n).half(), init=rn(n).half(), noise=rn(n).half(),
                mask=torch.rand(B * HW, generator=g, dtype=torch.float64).half(),
                ddim_coef=torch.stack([5.0 + 1.5 * row, 1.0123 + 0.01 * row, -0.0456 - 0.02 * row], 1).float(),          # {g, c_x, c_e} per row
                blend_coef=torch.stack([0.9 - 0.1 * row, 0.3 + 0.15 * row], 1).float(),                                  # {c0, c1} per row
                s=rn(n).float(), noise32=rn(n).float())


def _per_row(coef, B, per):
    return [f64(coef)[:, k].reshape(B, 1).expand(B, per).reshape(-1) for k in range(coef.shape[1])]


def ddim_ref(case, coef, guided=True):
    """misc.hip ddim_step_kernel: e = eu + g (ec - eu); out = fp16(c_x x + c_e e). coef fp32 [B, 3]. Roundings: ec - eu, its product with g, the sum e (2 |g d| + |e|);
    c_e e, c_x x, the sum"""
    g, cx, ce = _per_row(coef, case["B"], case["per"])
    x, eu, ec = f64(case["x"]), f64(case["eu"]), f64(case["ec"])
    if guided:
        d = ec - eu
        e = eu + g * d
        Ee = U * (2 * (g * d).abs() + e.abs())
    else:
        e, Ee = eu, torch.zeros_like(eu)
    out = cx * x + ce * e
    return out, with_store16(out, SECOND * (ce.abs() * Ee + U * ((ce * e).abs() + (cx * x).abs() + out.abs())))


def blend_ref(case, coef):
    """misc.hip mask_blend_kernel: keep = c0 init + c1 noise; out = fp16((1 - m) keep + m x), m the pixel's mask value shared by the C channels"""
    B, C, HW = case["B"], case["C"], case["HW"]
    c0, c1 = _per_row(coef, B, case["per"])
    m = f64(case["mask"]).reshape(B, 1, HW).expand(B, C, HW).reshape(-1)
    x, init, noise = f64(case["x"]), f64(case["init"]), f64(case["noise"])
    keep = c0 * init + c1 * noise
    Ek = U * ((c0 * init).abs() + (c1 * noise).abs() + keep.abs())
    out = (1 - m) * keep + m * x
    Bf = (1 - m).abs() * Ek + U * ((1 - m).abs() * keep.abs() + ((1 - m) * keep).abs() + (m * x).abs() + out.abs())
    return out, with_store16(out, SECOND * Bf)


PRIOR_SCALARS = dict(g=3.5, sqrt_a=0.83, sqrt_b=0.5578, k0=0.31, k1=0.64, sigma=0.21)


def prior_ref(case, guided=True, noisy=True):
    """misc.hip prior_step_kernel, fp32 in and out: eps_i = (s - sqrt_a o_i) / sqrt_b; eps = eps_u + g (eps_c - eps_u); x0 = (s - sqrt_b eps) / sqrt_a;
    out = k0 x0 + k1 s + sigma noise. A division counts 2 u (correctly rounded or a reciprocal and a product)"""
    p = {k: f32(v) for k, v in PRIOR_SCALARS.items()}
    s, oc, ou, nz = f64(case["s"]), f64(case["ec"]), f64(case["eu"]), f64(case["noise32"])

    def eps_of(o):
        t = s - p["sqrt_a"] * o
        e = t / p["sqrt_b"]
        return e, (U * ((p["sqrt_a"] * o).abs() + t.abs())) / p["sqrt_b"] + 2 * U * e.abs()
    e, Ee = eps_of(ou)
    if guided:
        ec, Ec = eps_of(oc)
        d = ec - e
        e2 = e + p["g"] * d
        Ee = Ee + abs(p["g"]) * (Ec + Ee) + U * (d.abs() * abs(p["g"]) + 2 * (p["g"] * d).abs() + e2.abs())
        e = e2
    t = s - p["sqrt_b"] * e
    x0 = t / p["sqrt_a"]
    E0 = (p["sqrt_b"] * Ee + U * ((p["sqrt_b"] * e).abs() + t.abs())) / p["sqrt_a"] + 2 * U * x0.abs()
    o = p["k0"] * x0 + p["k1"] * s
    Eo = abs(p["k0"]) * E0 + U * ((p["k0"] * x0).abs() + (p["k1"] * s).abs() + o.abs())
    if noisy:
        o2 = o + p["sigma"] * nz
        Eo = Eo + U * ((p["sigma"] * nz).abs() + o2.abs())
        o = o2
    return o, SECOND * Eo


# ---- the skinny linear -----------------------------------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = ((1, 50, 64), (16, 70, 128), (3, 13760, 64))
LINEAR_REAL_SHAPES = ((3, 50, 64), (16, 70, 128))


def linear_case(M, N, K, seed=None, real=False):
    g = gen(8000 + M + N + K if seed is None else seed)
    if real:
        X, W = torch.randn(M, K, generator=g, dtype=torch.float64), torch.randn(N, K, generator=g, dtype=torch.float64) * K ** -0.5
        bias = torch.randn(N, generator=g, dtype=torch.float64)
    else:
        X, W = ints((M, K), g), ints((N, K), g) * WUNIT
        bias = column_bias(N)
    return dict(M=M, N=N, K=K, A=X.half(), W=W.half(), bias=bias.half(), res=None, unit=WUNIT)


def linear_ref(case, silu_in=0, silu_out=0):
    """misc.hip linear_small_kernel: out = fp16(act(sum_k f(x_k) w_k + bias)). Flags 0 on the lattice: the exact bits. With the flags: f(x) carries the SiLU terms on an
    exact x; the sum of K products in any order K u sum |f(x) w| (llm_ops_ref), the bias one more rounding; the output SiLU as in silu_bound.
    -> (ref, bound, the modelled exponential's share)"""
    X, W, b = f64(case["A"]), f64(case["W"]), f64(case["bias"])
    K = X.shape[1]
    if not silu_in and not silu_out:
        return round16(X @ W.t() + b), None, 0.0
    Xm = torch.zeros_like(X)
    Ex = torch.zeros_like(X)
    if silu_in:
        X, Ex, Xm = silu_bound(X, torch.zeros_like(X))
    r = X @ W.t() + b
    E = Ex @ W.abs().t() + SECOND * ((K + 1) * U * (X.abs() @ W.abs().t()) + U * r.abs())
    Xpart = Xm @ W.abs().t()
    if silu_out:
        s = torch.sigmoid(r)
        Xpart = (s * (1 + r * (1 - s))).abs() * Xpart
        r, E, Xo = silu_bound(r, E)
        Xpart = Xpart + Xo
    total = with_store16(r, E)
    return r, total, float((Xpart / total).max())


# ---- the folded LayerNorm and the row statistics of its producer ----------------------------------------------------------------------------------------------
LNFOLD_SHAPES = ((77, 128, 132), (300, 256, 768))          # M, C (the normalised width = both K), N
LNFOLD_TILES = (-1, 0, 4, 6, 8, 11, 12, 20, 21)
LNFOLD_GEGLU_TILES = (18, 22, 27)


def lnfold_case(M, C, N, seed=None, geglu=False):
    """producer: X [M, C] in {-1, 0, 1}, Wp [C, C] in {-1, 0, 1} / 4, a residual constant along a row: 0 on three rows of four, +-(10 .. 13) times the row's standard
    deviation on the fourth (|mean| / std reaches 10) -- t = fp16(fp16(X Wp^T) + R) stays on the 1/4 lattice. consumer: W [N, C] on the 2^-8 lattice, gamma in
    {1, 2, 3} / 2 (W gamma is an fp16 value), beta = ((c % 11) - 5) / 8, a bias per column. geglu: N = 8 C' packed columns are the caller's business"""
    g = gen(9000 + M + C + N if seed is None else seed)
    X, Wp = ints((M, C), g, -1, 1), ints((C, C), g, -1, 1) * 0.25
    std = math.sqrt(C * (2.0 / 3.0) * (2.0 / 3.0)) * 0.25
    i = torch.arange(M)
    level = torch.where(i % 4 == 3, torch.where(i % 8 == 3, 1.0, -1.0) * torch.round((10.0 + (i % 4)) * std * 4) / 4, torch.zeros(M)).double()
    c = torch.arange(C)
    W = ints((N, C), g) * (2.0 ** -6 if geglu else WUNIT)
    bias = torch.cat([(torch.arange(N // 2) % 29 - 14).double() * 2.0 ** -3, (torch.arange(N // 2) % 37 - 18).double() * 0.125]) if geglu else column_bias(N)
    return dict(M=M, C=C, N=N, X=X.half(), Wp=Wp.half(), R=level.reshape(M, 1).expand(M, C).contiguous().half(), W=W.half(), gamma=((1 + c % 3).double() / 2).half(),
                beta=(((c % 11) - 5).double() / 8).half(), bias=bias.half(), eps=1e-5)


def lnfold_producer(case):
    """-> t [M, C] (the exact fp16 output) and its row statistics {sum, sum of squares} [M, 2] in fp64: the slots of a launch must add up to exactly these"""
    t = round16(round16(f64(case["X"]) @ f64(case["Wp"]).t()) + f64(case["R"]))
    return t, torch.stack([t.sum(1), (t * t).sum(1)], 1)


def lnfold_weights(case):
    """ia2p_fold_layernorm (misc.hip fold_ln_kernel): Wf = fp16(W gamma) (exact by construction: to the bit), cs = sum_k Wf (a lattice sum: exact),
    lb = bias + sum_k W beta with its plain fp32 bound (K + 1) u sum |W beta| + u |lb| -> Wf, cs, (lb, bound)"""
    W, ga, be, b = f64(case["W"]), f64(case["gamma"]), f64(case["beta"]), f64(case["bias"])
    Wf = W * ga
    assert torch.equal(Wf, round16(Wf))
    lb = b + W @ be
    return Wf, Wf.sum(1), (lb, SECOND * ((W.shape[1] + 1) * U * (W.abs() @ be.abs()) + U * lb.abs()))


def lnfold_ref(case, t, stats=None):
    """LayerNorm(t) . W^T + bias in fp64 and the fp32 bound of the folded epilogue (docstring) -> (h [M, N], fp32 bound E): the caller adds the fp16 store or GEGLU.
    stats [M, 2]: other {sum, sum of squares} than the rows' own (the mutants of test_unet_ops_cpu.py)"""
    t = f64(t)
    K = t.shape[1]
    Wf, cs, (lb, Elb) = lnfold_weights(case)
    s1, s2 = (t.sum(1, keepdim=True), (t * t).sum(1, keepdim=True)) if stats is None else (stats[:, :1], stats[:, 1:])
    mean = s1 / K
    var = s2 / K - mean * mean
    w = var + f32(case["eps"])
    inv_err = 0.0 if K & (K - 1) == 0 else U
    dm = U * mean.abs() + inv_err * mean.abs()
    dv = 3 * U * mean * mean + U * var + inv_err * s2 / K
    assert bool((dv < 0.5 * w).all())
    rstd = w ** -0.5
    r = (1 - dv / w) ** -0.5 - 1 + 3 * U
    acc = t @ Wf.t()
    inner = acc - mean * cs
    Ein = dm * cs.abs() + U * inner.abs()
    h = rstd * inner + lb
    E = SECOND * (rstd * (inner.abs() * r + Ein) + Elb + U * h.abs())
    return h, E


def lnfold_exactness(case, t):
    """largest partial-sum magnitude of producer and consumer accumulators in their lattice units (2^-2 and 2^-11 for the consumer: t in 1/4, Wf in 2^-9)"""
    Wf = lnfold_weights(case)[0]
    return max(float((f64(case["X"]).abs() @ f64(case["Wp"]).abs().t() + f64(case["R"]).abs()).max()) * 4, float((f64(t).abs() @ Wf.abs().t()).max()) * 2.0 ** 11,
               float((f64(t) ** 2).sum(1).max()) * 16)
