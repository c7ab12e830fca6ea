"""fp64 references of the GEMM and 3x3-convolution options that only the encoders, the VAE and the context projection set -- the activations (`act` 1 / 2 / 3, alone
and behind a folded LayerNorm), the epilogue scales, operand strides, the row map, a column block of a wider output, `pad_lo = 0` -- and next to each the bound the
launch must meet (None: the exact bits). They go through `ia2p_gemm_form` / `ia2p_conv3x3_form`. Written in the manner of unet_ops_ref.py, whose helpers it imports
and whose notation it keeps: u = 2^-24, SECOND covers second-order terms. Every bound is derived from the operations read in csrc/gemm_epilogue.h, gemm.hip
(splitk_reduce_kernel) and common.h (act_f), or measured on the CPU against fp64; none comes from a kernel's output.

  lattice       as unet_ops_ref: operands are integers in [-3, 3] times a power of two, so the accumulator is the fp64 sum in any order (`exactness(case)` < 2^24, asserted for
                every case in test_encoder_gemm_cpu.py). Every step behind it is one stated fp32 operation:
                  1. v = fl(acc e_as)                    (`v *= e_as`)
                  2. v = fl(bias e_bs + v)               (`fmaf(bias, e_bs, v)`; a folded LayerNorm replaces 1 and 2: unet_ops_ref.lnfold_ref)
                  3. v = act(v)
                  4. v = fp16(v)                         only where a row vector or a residual follows
                  5. v = fl(rowvec e_bs + v)             (`fmaf`)
                  6. v = fl(v + residual)
                  7. out = fp16(v)
                The same seven lines stand in the register epilogue (no activation there), in both forms of the fp32-tile route and in the reduce kernel.
  no activation a product of an fp32 value and an fp32 scale and an fma are correctly rounded operations, and nothing around them can be contracted (the product feeds the
                fma's addend): the reference performs 1 .. 7 in fp64 with the roundings spelled out (`round32`, `round16`) and the launch must give its BITS -- on the
                lattice with power-of-two scales no fp32 step rounds at all; with e_as = 1 / sqrt(512), 1 / sqrt(128) (no bias: the VAE's scores) step 1 is the one
                correctly rounded fp32 product of an exact accumulator.
  activations   the pre-activation v is exact (a lattice sum), or known to within E behind a folded LayerNorm (|act'| <= 1.13 for all three: 1.13 E reaches the result).
                The reference is act(v) in fp64; the bound is the formula's own fp32 error and half an fp16 ulp (`with_store16`); where a row vector or a residual follows,
                that bound with its fp16 rounding (4), the two fp32 roundings of 5 and 6 (u each, on the magnitudes they produce) and the store.
    act 1       gelu_erf_f: encoder_ops_ref's derivation (docs/LOG.md §25.1): 0.5 |v| (GELU_ERF_CPU + 11 u) + 4 u |gelu|, GELU_ERF_CPU = 5.6e-7 the error of the
                Abramowitz-Stegun polynomial in numpy fp32, measured again here over every pre-activation the cases use. MODELLED inside the 11 u: the hardware
                reciprocal (1 ulp of t <= 1 through a polynomial of slope <= 1.3: 3 u) and the native exponential ((z^2 + 4) 2^-23 relative); both reach erf multiplied by
                exp(-z^2) resp. erfc(|z|), z = v / sqrt 2: M = 0.5 |v| (3 u exp(-z^2) + 2 u (z^2 + 4) erfc(|z|)) (11 u at z = 0, as §25.1 says).
    act 2       quick_gelu_f = v rcp(1 + __expf(-1.702f v)); reference v sigmoid(1.702 v). a = fl(-1.702f v): the constant's rounding and the product, 2 u |a|, an absolute
                error of the exponential's argument = a relative one of e = exp(a); e reaches sigmoid = 1 / (1 + e) multiplied by 1 - sigmoid. 1 + e: u; v r: u. Counted:
                |ref| ((1 - s) 2 u |a| + 2 u). MODELLED: __expf off by (|a| + 4) 2^-23 relatively and the 1-ulp reciprocal (2 u): M = |ref| ((1 - s) 2 u (|a| + 4) + 2 u).
                Beyond a = 88.7 __expf overflows, the reciprocal of infinity is 0 and the result -0: the reference is below 60 exp(-88) there, and results below 2^-126 may
                be flushed: + 1e-36.
    act 3       gelu_tanh_f = 0.5 v (1 + tanhf(c0 (v + c1 v^3))), c0 = sqrt(2 / pi), c1 = 0.044715; reference v sigmoid(2 c0 (v + c1 v^3)) (= the same, without the
                cancellation of 1 + tanh). t1 = c1 v^3: two products, the constant, its product: 4 u |t1|; inner = v + t1: u |inner|; arg = c0 inner: the constant and the
                product, 2 u |arg|: E_arg = c0 (4 u |t1| + u |inner|) + 2 u |arg|, which reaches tanh multiplied by sech^2(arg). 1 + tanh: u (1 + tanh); the two products:
                2 u |ref|. MODELLED: the device library's tanhf within 2 ulp, T = 2^-22 |tanh|: M = 0.5 |v| T.
  the tenth     the modelled terms cannot be checked without the hardware; the project's standing condition is that they stay below a tenth of the bound of every
                element (`form_ref` returns M / bound; the CPU file asserts it). It holds for act 1 and act 2 everywhere. For act 3 it CANNOT hold in the negative
                tail, and the CPU file asserts it for v >= TANH_TENTH_FROM = -2.5 only: below, 1 + tanhf is the difference of 1 and a value one fp32 step from -1, so the
                formula's whole fp32 error IS the library's last bits of tanhf (0.5 |v| 2^-22 against an fp16 half ulp that shrinks with Phi(v)). The bound there is the
                2-ulp model itself, at most 0.5 * 6.5 * 2^-22 = 7.8e-7 in absolute terms; docs/LOG.md §42.4 says so.
  coverage      a condition on the inputs, asserted on the CPU for every activation case: at least a quarter of the pre-activations in [-6.5, -0.25] and a quarter in
                [0.25, 6.5]; with a bias, columns 0 / 2 / 3 / 5 carry +12 / -12 / +60 / -60 (saturation: __expf overflow, -0 results) and every third column a bias in
                [48, 64), where fp16 steps by 2^-5. The other biases are multiples of 2^-11 in [-1, 1), each column its own: pre-activations between 1 and 8 are then NO
                fp16 values, so an activation applied after an fp16 rounding is another result.
  strides, row map   the case holds the operands as the launch reads them -- flat fp16 storage, an offset and a row stride each, NaN wherever the launch must not read -- and
                `logical(case)` gathers A, W and the residual through the descriptor's own arithmetic (row(m) = (m / rpb) bstride + m % rpb + roff). A planted fault is
                the same gather with one field changed.
  convolution   unet_ops_ref's lattice with `pad_lo` zero rows / columns in front of the image and one behind it; steps 1 .. 7 as above: the exact bits.
  real values   (the transformer-block round) a sum of K products in fp32 in any order: (K + 1) u sum |a w|, the bias one more u (llm_ops_ref); the folded LayerNorm of
                unet_ops_ref.lnfold_ref with the summation error of the producer's fp32 row statistics added: H u sum |x| on the sum, (H + 1) u sum x^2 on the squares.
"""
import math

import numpy as np
import torch

from llm_ops_ref import SECOND, U, f64, half_ulp16  # noqa: F401
from encoder_ops_ref import GELU_ERF_CPU, erf_poly32, round16, with_store16  # noqa: F401
from unet_ops_ref import (CONV_AXES, LNFOLD_TILES, WUNIT, accept, exactness, f32, gen, ints, lnfold_case, lnfold_producer, lnfold_ref, lnfold_weights,  # noqa: F401
                          row_residual, scrambled_fp32_sum, worst)

SQRT2 = math.sqrt(2.0)
C_QUICK = 1.702
C_TANH0, C_TANH1 = 0.79788456080286535588, 0.044715
TANH_TENTH_FROM = -2.5
ACT_LIPSCHITZ = 1.13
ACTS = (1, 2, 3)
IN_LAUNCH, REDUCE_LAUNCH = 1 << 40, 0          # ia2p_debug_set_splitk_inkernel: every K split finishes in its launch / none does


def round32(x):
    """the correctly rounded fp32 values of an fp64 tensor, as fp64"""
    return torch.from_numpy(f64(x).numpy().astype(np.float32).astype(np.float64))


# ---- activations ---------------------------------------------------------------------------------------------------------------------------------------------
def act64(v, act):
    v = f64(v)
    if act == 1:
        return 0.5 * v * torch.special.erfc(-v / SQRT2)
    if act == 2:
        return v * torch.sigmoid(C_QUICK * v)
    if act == 3:
        return v * torch.sigmoid(2.0 * C_TANH0 * (v + C_TANH1 * v * v * v))
    return v


def act_bound(v, act):
    """-> (act(v), the fp32 bound B of the kernel's formula at an exact v, the modelled part M of B) -- docstring"""
    v = f64(v)
    ref = act64(v, act)
    if act == 1:
        z2 = 0.5 * v * v
        M = 0.5 * v.abs() * (3 * U * torch.exp(-z2) + 2 * U * (z2 + 4) * torch.special.erfc(v.abs() / SQRT2))
        return ref, SECOND * (0.5 * v.abs() * (GELU_ERF_CPU + 11 * U) + 4 * U * ref.abs()), M
    if act == 2:
        a = (C_QUICK * v).abs()
        s = torch.sigmoid(C_QUICK * v)
        M = ref.abs() * ((1 - s) * 2 * U * (a + 4) + 2 * U)
        return ref, SECOND * (ref.abs() * ((1 - s) * 2 * U * a + 2 * U) + M) + 1e-36, M
    if act == 3:
        t1 = C_TANH1 * v * v * v
        inner = v + t1
        arg = C_TANH0 * inner
        s = torch.sigmoid(2.0 * arg)
        one, sech2, th = 2.0 * s, 4.0 * s * (1 - s), 2.0 * s - 1.0
        E_arg = C_TANH0 * (4 * U * t1.abs() + U * inner.abs()) + 2 * U * arg.abs()
        M = 0.5 * v.abs() * 2.0 ** -22 * th.abs()
        return ref, SECOND * (0.5 * v.abs() * (sech2 * E_arg + U * one) + 2 * U * ref.abs() + M), M
    return ref, torch.zeros_like(ref), torch.zeros_like(ref)


def act32(v, act):
    """the kernel's formula in numpy fp32, one rounding per operation (a true division and numpy's exp / tanh where the kernel takes the hardware's and the library's)"""
    f = np.float32
    x = f64(v).numpy().astype(np.float32)
    assert np.array_equal(x.astype(np.float64), f64(v).numpy()), "the pre-activations must be fp32 values"
    with np.errstate(over="ignore"):
        if act == 1:
            r = f(0.5) * x * (f(1) + erf_poly32(x * f(0.70710678118654752440)))
        elif act == 2:
            r = x * (f(1) / (f(1) + np.exp(f(-1.702) * x)))
        elif act == 3:
            r = f(0.5) * x * (f(1) + np.tanh(f(C_TANH0) * (x + f(C_TANH1) * x * x * x)))
        else:
            r = x
    assert r.dtype == np.float32
    return torch.from_numpy(r.astype(np.float64))


# ---- the epilogue behind the pre-activation: steps 3 .. 7 ------------------------------------------------------------------------------------------------------
def epilogue_ref(v, E, act=0, rowvec=None, res=None, e_bs=1.0, fault=None):
    """v: the value in front of step 3 (fp64), exact (E None) or within E. rowvec, res: [M, N] fp64 or None (the row vector already expanded to rows).
    -> (ref, bound or None for the exact bits, the modelled terms' share of the bound element by element or None). fault: a planted fault of test_encoder_gemm_cpu.py (a name)"""
    v = f64(v)
    tail = rowvec is not None or res is not None
    rv = None if rowvec is None else f64(rowvec) * (1.0 if fault == "rowvec unscaled" else e_bs)
    rs = None if res is None else f64(res) * (e_bs if fault == "residual scaled" else 1.0)
    if not act and E is None:
        h = round16(v) if tail else v
        if rv is not None:
            h = round32(rv + h)
        if rs is not None:
            h = round32(h + rs)
        return round16(h), None, None
    if fault == "act after the fp16 rounding":
        v = round16(v)
    if fault == "act after the residual":
        return round16(act64(round16(v) + (0 if rv is None else rv) + (0 if rs is None else rs), act)), None, 0.0
    ref, B, M = act_bound(v, act)
    if E is not None:
        B = B + SECOND * ACT_LIPSCHITZ * f64(E) if act else f64(E)
    if not tail:
        bound = with_store16(ref, B)
        return ref, bound, M / bound
    E1 = with_store16(ref, B)
    s1 = ref if rv is None else ref + rv
    s = s1 if rs is None else s1 + rs
    bound = with_store16(s, E1 + SECOND * U * ((s1.abs() if rv is not None else 0) + (s.abs() if rs is not None else 0)))
    return s, bound, M / bound


# ---- a GEMM form: logical operands or strided storage ------------------------------------------------------------------------------------------------------------
def row_map(M, rpb, bstride, roff):
    m = torch.arange(M)
    return m if rpb == 0 else (m // rpb) * bstride + m % rpb + roff


def _rows(flat, off, ld, rows, width):
    return flat[(off + rows.reshape(-1, 1) * ld + torch.arange(width).reshape(1, -1)).reshape(-1)].reshape(len(rows), width)


def logical(c, **over):
    """A [M, K], W [N, K], residual [M, N] or None as the descriptor of `c` (with the fields in `over` changed: the planted faults) reads them from the case's storage"""
    d = dict(c, **over)
    A = _rows(f64(c["A_flat"]), d["a_off"], d["lda"], row_map(d["M"], d["rpb"], d["bstride"], d["roff"]), d["K"])
    W = _rows(f64(c["W_flat"]), d["w_off"], d["ldw"], torch.arange(d["N"]), d["K"])
    R = None if c.get("R_flat") is None else _rows(f64(c["R_flat"]), 0, d["ldr"], torch.arange(d["M"]), d["N"])
    return A, W, R


def _store(rows_at, X, ld, tail=8, min_rows=0):
    """X [R, w] at rows `rows_at` of a NaN-filled flat fp16 buffer of row stride ld (at least min_rows rows)"""
    n = max(int(rows_at.max()) * ld + X.shape[1], min_rows * ld) + tail
    flat = torch.full((n,), float("nan"), dtype=torch.float16)
    idx = rows_at.reshape(-1, 1) * ld + torch.arange(X.shape[1]).reshape(1, -1)
    flat[idx.reshape(-1)] = X.half().reshape(-1)
    return flat


def act_bias(N):
    """docstring "coverage": +-12 and +-60 on columns 0 / 2 / 3 / 5, 48 + (j % 448) / 32 on every third column, multiples of 2^-11 in [-1, 1) elsewhere, each its own"""
    j = torch.arange(N)
    b = (((j * 1237) % 4096) - 2048).double() * 2.0 ** -11
    b = torch.where(j % 3 == 1, 48.0 + (j % 448).double() * 2.0 ** -5, b)
    for col, val in ((0, 12.0), (2, -12.0), (3, 60.0), (5, -60.0)):
        b[col] = val
    return b


def rowvec_rows(nb, N, g):
    b, n = torch.arange(nb).reshape(nb, 1), torch.arange(N).reshape(1, N)
    return (b + 1).double() * 0.5 + (n % 8).double() * 2.0 ** -6 + ints((nb, N), g) * WUNIT


def form_case(M, N, K, unit=WUNIT, bias="column", res=False, rowvec=0, act=0, e_as=1.0, e_bs=1.0, lda=None, ldw=None, ldr=None, ldc=None, col0=0, rowmap=(0, 0, 0),
              shared=False, seed=None, tag=""):
    """one launch of ia2p_gemm_form on the lattice. bias: "column" (unet_ops_ref.column_bias), "act" (act_bias) or None; rowvec: rows per batch (0: none); shared: A and W
    are the two halves of one [M, 2 K] tensor (N == M: the VAE's score launch)"""
    from unet_ops_ref import column_bias
    g = gen(11000 + M + 3 * N + 7 * K if seed is None else seed)
    A, W = ints((M, K), g), ints((N, K), g) * unit
    rpb, bstride, roff = rowmap
    lda, ldw, ldr, ldc = lda or K, ldw or K, ldr or N, ldc or N
    c = dict(tag=tag, M=M, N=N, K=K, unit=min(unit, 2.0 ** -11) * min(1.0, 2.0 ** math.floor(math.log2(min(e_as, e_bs)))), act=act, e_as=f32(e_as), e_bs=f32(e_bs),
             lda=lda, ldw=ldw, ldr=ldr, ldc=ldc, col0=col0, rpb=rpb, bstride=bstride, roff=roff, a_off=0, w_off=0, rows_per_batch=rowvec)
    if shared:
        assert N == M and lda == ldw == 2 * K
        c["A_flat"] = c["W_flat"] = torch.cat([A, W], 1).half().reshape(-1)
        c["w_off"] = K
    else:
        c["A_flat"] = _store(row_map(M, rpb, bstride, roff), A, lda, min_rows=(M // rpb) * bstride + 8 if rpb else 0)      # (the whole [B, L, K] tensor and a few rows)
        c["W_flat"] = _store(torch.arange(N), W, ldw)
    c["bias"] = None if bias is None else (act_bias(N) if bias == "act" else column_bias(N)).half()
    c["R_flat"] = _store(torch.arange(M), row_residual(M, N, g), ldr) if res else None
    c["rowvec"] = rowvec_rows((M + rowvec - 1) // rowvec, N, g).half() if rowvec else None
    c["A"], c["W"], R = logical(c)          # (what `exactness` reads)
    c["A"], c["W"], c["res"] = c["A"].half(), c["W"].half(), None if R is None else R.half()
    return c


def pre_activation(c, A=None, W=None, fault=None):
    """steps 1 and 2 -> (v, True where no fp32 step rounded: v is then the exact acc e_as + bias e_bs)"""
    A0, W0, _ = logical(c)
    acc = f64(A0 if A is None else A) @ f64(W0 if W is None else W).t()
    b = None if c["bias"] is None else f64(c["bias"]) * c["e_bs"]
    if fault == "acc_scale after the bias":
        v = round32((acc + (0 if b is None else f64(c["bias"]))) * c["e_as"])
        return v, False
    v0 = acc * c["e_as"]
    v = round32(v0)
    exact = bool((v == v0).all())
    if b is not None:
        v1 = v + b
        v = round32(v1)
        exact = exact and bool((v == v1).all())
    return v, exact


def form_ref(c, fault=None, **over):
    """-> (ref [M, N], bound or None, share). over: descriptor fields read differently (planted faults)"""
    A, W, R = logical(c, **over)
    v, exact = pre_activation(c, A, W, fault)
    assert exact or not c["act"] or fault, "an activation case must have an exact pre-activation"
    rv = None if c["rowvec"] is None else f64(c["rowvec"])[torch.arange(c["M"]) // c["rows_per_batch"]]
    act = c["act"]
    if fault == "act 1 <-> 3":
        act = {1: 3, 3: 1}[act]
    ref, bound, share = epilogue_ref(v, None, act, rv, R, c["e_bs"], fault)
    if fault in ("1.7 for 1.702", "A&S coefficient") and bound is not None:
        ref = _act_variant(v, fault)
        if rv is not None or R is not None:
            ref = ref + (0 if rv is None else rv * c["e_bs"]) + (0 if R is None else R)
    return ref, bound, share


def _act_variant(v, fault):
    """a formula with one constant changed, in fp64"""
    v = f64(v)
    if fault == "1.7 for 1.702":
        return v * torch.sigmoid(1.7 * v)
    z = (v / SQRT2).abs()                      # Abramowitz-Stegun 7.1.26 with p = 0.3275912 (the last digit of 0.3275911 off by one)
    t = 1.0 / (1.0 + 0.3275912 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    erf = torch.sign(v) * (1.0 - poly * torch.exp(-z * z))
    return 0.5 * v * (1.0 + erf)


def coverage(v):
    """-> (share of the pre-activations in [-6.5, -0.25], share in [0.25, 6.5])"""
    v = f64(v)
    return float(((v >= -6.5) & (v <= -0.25)).double().mean()), float(((v >= 0.25) & (v <= 6.5)).double().mean())


# ---- the GPU cases ---------------------------------------------------------------------------------------------------------------------------------------------------
ACT_UNIT = {64: 2.0 ** -4, 128: 2.0 ** -4, 640: 2.0 ** -5}
ACT_SHAPES = ((37, 64, 64), (77, 132, 128), (130, 200, 640), (300, 768, 128))          # N = 132: N % 8 == 4, the 8-byte form of the fp32-tile route
ACT_TILES = LNFOLD_TILES                                                                 # -1 and one variant of every epilogue family
ACT_EPILOGUES = tuple((b, r) for b in (True, False) for r in ("none", "residual", "aliased residual"))
ACT_SPLITS = {640: (2, 5), 128: (2,), 64: ()}


def act_case(M, N, K, act, bias=True, res=False, ldc=None):
    return form_case(M, N, K, unit=ACT_UNIT[K], bias="act" if bias else None, res=res, act=act, ldc=ldc, seed=12000 + M + N + K, tag=f"act {act} {M}x{N}x{K}")


LN_ACT_SHAPES = ((77, 128, 132), (300, 256, 768))


def ln_act_case(M, C, N):
    """unet_ops_ref.lnfold_case (a quarter of the rows at |mean| / std = 10 .. 13) with a bias of its own: 48 + (j % 448) / 32 on every third column, multiples of 2^-9
    spread over [-3, 3) on the others (the normalised rows give sums of about 0.1: the bias places the pre-activations), and the saturation columns of `act_bias`"""
    c = lnfold_case(M, C, N)
    j = torch.arange(N)
    b = torch.where(j % 3 == 1, 48.0 + (j % 448).double() * 2.0 ** -5, (((j * 1237) % 3072) - 1536).double() * 2.0 ** -9)
    for col, val in ((0, 12.0), (2, -12.0), (3, 60.0), (5, -60.0)):
        b[col] = val
    c["bias"] = b.half()
    return c


def ln_act_ref(c, t, act):
    h, E = lnfold_ref(c, t)
    ref, bound, share = epilogue_ref(h, E, act)
    return ref, bound, share, h


SCALE_SHAPES = ((77, 200, 128, 11), (130, 132, 640, 13))          # M, N, K, rows per batch of the row vector; N = 200: the register route, N = 132: the fp32-tile route
SCALE_FORMS = (("as = bs = 2^-3", 2.0 ** -3, 2.0 ** -3, True, True), ("bs = 2^-2 alone", 1.0, 2.0 ** -2, True, True),
               ("as = 1 / sqrt(512), no bias", 512.0 ** -0.5, 1.0, False, False), ("as = 1 / sqrt(128), no bias", 128.0 ** -0.5, 1.0, False, False))
SCALE_TILES = (-1, 0, 4, 12, 20)


def scale_case(M, N, K, rpbatch, form):
    name, e_as, e_bs, bias, tail = form
    return form_case(M, N, K, bias="column" if bias else None, res=tail, rowvec=rpbatch if tail else 0, e_as=e_as, e_bs=e_bs, seed=13000 + M + N + K, tag=f"{name} {M}x{N}x{K}")


def stride_cases():
    """name -> case: the strides the executors set (docstring of include/ia2p.h ia2p_gemm_form)"""
    K = 128
    return {
        "scores: A and W the halves of one [M, 2 K] tensor": form_case(132, 132, K, bias=None, e_as=128.0 ** -0.5, lda=2 * K, ldw=2 * K, shared=True, seed=14001),
        "lda = 5 K": form_case(77, 200, K, lda=5 * K, ldw=K + 8, res=True, seed=14002),
        "ldc = 3 N + 8, col0 = N": form_case(130, 132, K, ldc=3 * 132 + 8, col0=132, res=True, seed=14003),
        "ldr = N + 4": form_case(77, 200, K, ldr=204, res=True, seed=14004),
        "M < N, ldc = 3 N + 8 (V^T)": form_case(37, 200, 64, ldc=608, col0=200, bias=None, seed=14005),
    }


ROWMAP_SHAPES = {"text rows (77, 81, 0)": (3 * 77, (77, 81, 0), 128), "image-token rows (4, 81, 77)": (3 * 4, (4, 81, 77), 128), "rpb = 1": (3, (1, 81, 5), 128),
                 "roff = 65535": (6, (2, 3, 65535), 64), "rpb = 65535": (65540, (65535, 65536, 1), 64)}
ROWMAP_REFUSED = ((65536, 65536, 0), (4, 81, 65536))


def rowmap_case(name):
    M, rm, K = ROWMAP_SHAPES[name]
    return form_case(M, 64 if K == 64 else 132, K, rowmap=rm, res=M < 1000, seed=15000 + M, tag=name)


# ---- the 3x3 convolution with pad_lo and the scales -------------------------------------------------------------------------------------------------------------
CONV_PAD0 = ((1, 10, 14, 64, 64), (2, 9, 7, 64, 72), (1, 16, 16, 64, 64))          # B, H, W, Cin, Co: stride 2, pad_lo 0, bias_scale 2^-2 (the VAE encoder's downsample)
CONV_UP = (2, 8, 8, 64, 64)                                                           # up 1, bias_scale 2^-2 (the VAE decoder's upsample)
CONV_SCALED = (1, 16, 16, 64, 160)                                                    # acc_scale = bias_scale = 2^-3 with a residual: halo-staged tiles 24 .. 26 and the gathered ones


def conv_out_hw(H, W, stride, up, pad_lo):
    Hv, Wv = H << up, W << up
    return (Hv + pad_lo + 1 - 3) // stride + 1, (Wv + pad_lo + 1 - 3) // stride + 1


def conv_form_case(B, H, W, Cin, Co, stride=1, up=0, pad_lo=1, e_as=1.0, e_bs=1.0, rowvec=True, res=True):
    from unet_ops_ref import column_bias
    g = gen(16000 + B + 3 * H + 5 * W + Cin + Co + stride + up + pad_lo)
    Ho, Wo = conv_out_hw(H, W, stride, up, pad_lo)
    c = dict(B=B, H=H, W=W, Cin=Cin, Co=Co, stride=stride, up=up, pad_lo=pad_lo, Ho=Ho, Wo=Wo, e_as=f32(e_as), e_bs=f32(e_bs), unit=WUNIT * min(e_as, e_bs, 1.0),
             x=ints((B, H, W, Cin), g).half(), w=(ints((Co, Cin, 3, 3), g) * WUNIT).half(), bias=column_bias(Co).half())
    p = torch.arange(Ho * Wo).reshape(1, Ho, Wo, 1)
    c["tv"] = rowvec_rows(B, Co, g).half() if rowvec else None
    c["res"] = (((p % 13) - 6).double() * 0.5 + ints((B, Ho, Wo, Co), g) * WUNIT).half() if res else None
    return c


def conv_form_sum(x, w, stride, up, pad_lo, trailing="zero"):
    """[B, Ho, Wo, Co] in fp64: nine shifted matrix products over the image with pad_lo zero rows / columns in front and one behind. trailing = "edge": the planted
    fault -- the row and the column behind the image repeat its last ones"""
    x, w = f64(x), f64(w)
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, Ci = x.shape
    xp = torch.zeros(B, H + pad_lo + 1, W + pad_lo + 1, Ci, dtype=torch.float64)
    xp[:, pad_lo:pad_lo + H, pad_lo:pad_lo + W] = x
    if trailing == "edge":
        xp[:, pad_lo + H] = xp[:, pad_lo + H - 1]
        xp[:, :, pad_lo + W] = xp[:, :, pad_lo + W - 1]
    Ho, Wo = (H + pad_lo - 2) // stride + 1, (W + pad_lo - 2) // stride + 1
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] @ w[:, :, ky, kx].t()
    return out


def conv_form_exactness(c):
    a = conv_form_sum(f64(c["x"]).abs(), f64(c["w"]).abs(), c["stride"], c["up"], c["pad_lo"]) + f64(c["bias"]).abs()
    if c["tv"] is not None:
        a = a + f64(c["tv"]).abs()[:, None, None, :]
    if c["res"] is not None:
        a = a + f64(c["res"]).abs()
    return float(a.max()) / c["unit"]


def conv_form_ref(c, pad_lo=None, trailing="zero", fault=None):
    """-> (ref [B, Ho, Wo, Co], None): the exact bits. pad_lo / trailing / fault: the planted faults"""
    acc = conv_form_sum(c["x"], c["w"], c["stride"], c["up"], c["pad_lo"] if pad_lo is None else pad_lo, trailing)
    assert tuple(acc.shape[1:3]) == (c["Ho"], c["Wo"])
    v = round32(round32(acc * c["e_as"]) + f64(c["bias"]) * c["e_bs"])
    tv = None if c["tv"] is None else f64(c["tv"])[:, None, None, :].expand_as(v)
    ref, bound, _ = epilogue_ref(v, None, 0, tv, c["res"], c["e_bs"], fault)
    return ref, bound


# ---- one pre-LayerNorm transformer block on real values (csrc/xf_layer.h) -----------------------------------------------------------------------------------------
XF = dict(M=77, H=128, I=512, eps=1e-5)


def xf_case(seed=17000):
    g = gen(seed)
    H, I, M = XF["H"], XF["I"], XF["M"]
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    c = dict(XF, x=(rn(M, H) * 1.5 + 0.3).half(), att=rn(M, H).half())
    for name, n, k in (("qkv", 3 * H, H), ("o", H, H), ("fc1", I, H), ("fc2", H, I)):
        c["w_" + name] = (rn(n, k) * k ** -0.5).half()
        c["b_" + name] = (rn(n) * 0.5).half()
    for name in ("ln1", "ln2"):
        c[name + "_g"] = (1.0 + 0.25 * rn(H)).half()
        c[name + "_b"] = (0.25 * rn(H)).half()
    return c


def real_gemm(A, W, bias):
    """-> (A W^T + bias in fp64, the fp32 bound of a sum of K products in any order and the bias)"""
    A, W = f64(A), f64(W)
    v = A @ W.t() + (0 if bias is None else f64(bias))
    return v, SECOND * U * ((A.shape[1] + 1) * (A.abs() @ W.abs().t()) + (0 if bias is None else f64(bias).abs()) + v.abs())


def real_lnfold(t, Wf, cs, lb, eps):
    """the folded LayerNorm of unet_ops_ref.lnfold_ref on real values: t [M, K] the stored rows (fp16), Wf, cs, lb the folded weight (fp16), column sums and folded
    bias AS THE FOLD LAUNCH LEFT THEM (fp32: taken as given). The row statistics are the producer's fp32 sums of K terms: K u sum |t| and (K + 1) u sum t^2 reach mean
    and variance; the accumulator is a real fp32 sum: (K + 1) u sum |t Wf| -> (h, E)"""
    t, Wf, cs, lb = f64(t), f64(Wf), f64(cs), f64(lb)
    K = t.shape[1]
    s1, s2 = t.sum(1, keepdim=True), (t * t).sum(1, keepdim=True)
    d1, d2 = K * U * t.abs().sum(1, keepdim=True), (K + 1) * U * s2
    mean = s1 / K
    var = s2 / K - mean * mean
    w = var + f32(eps)
    inv_err = 0.0 if K & (K - 1) == 0 else U
    dm = d1 / K + (U + inv_err) * mean.abs()
    dv = d2 / K + 2 * mean.abs() * dm + 3 * U * mean * mean + U * var + inv_err * s2 / K
    assert bool((dv < 0.5 * w).all())
    rstd = w ** -0.5
    r = (1 - dv / w) ** -0.5 - 1 + 3 * U
    acc = t @ Wf.t()
    Eacc = (K + 1) * U * (t.abs() @ Wf.abs().t())
    inner = acc - mean * cs
    Ein = Eacc + dm * cs.abs() + U * inner.abs()
    h = rstd * inner + lb
    return h, SECOND * (rstd * (inner.abs() * r + Ein) + U * h.abs())


def row_stats_ref(x16, B):
    """{sum, sum of squares} [M, 2] of the stored fp16 rows and the bound of an fp32 sum of H terms in any order"""
    x = f64(x16)
    H = x.shape[1]
    st = torch.stack([x.sum(1), (x * x).sum(1)], 1)
    return st, SECOND * torch.stack([H * U * x.abs().sum(1), (H + 1) * U * (x * x).sum(1)], 1)


# ---- what the two entry points refuse on the host (both test files walk these lists; the CPU file with pointers that are never dereferenced) ---------------------------
INVALID, SHAPE = 1, 2          # IA2P_ERR_INVALID, IA2P_ERR_SHAPE (include/ia2p.h); a failed launch would be IA2P_ERR_HIP (6)
INF, NAN = float("inf"), float("nan")
GEMM_REFUSAL_BASE = dict(M=64, N=64, K=128, lda=128, ldw=128, ldr=64, ldc=64, rowvec_ld=64, rows_per_batch=16)      # every pointer set and aligned, no ln, no K split
# (what, fields set -- ("+", n): the pointer moved by n bytes, "ln.<field>": a complete ia2p_ln_fold with that field changed --, the status)
GEMM_REFUSALS = (
    ("A null", dict(A=0), INVALID), ("W null", dict(W=0), INVALID), ("C null", dict(C=0), INVALID), ("a K split without slabs", dict(splitk=2, partial=0), INVALID),
    ("M < 1", dict(M=0), SHAPE), ("N % 4", dict(N=62), SHAPE), ("N < 4", dict(N=0), SHAPE), ("K % 64", dict(K=96), SHAPE), ("K < 64", dict(K=0), SHAPE),
    ("lda < K", dict(lda=120), SHAPE), ("ldw < K", dict(ldw=64), SHAPE), ("ldc < N", dict(ldc=60), SHAPE), ("ldr < N", dict(ldr=32), SHAPE),
    ("rowvec_ld < N", dict(rowvec_ld=8), SHAPE), ("rows_per_batch < 1", dict(rows_per_batch=0), SHAPE),
    ("act 4 (ia2p_gemm_rowscale's)", dict(act=4), INVALID), ("act 5", dict(act=5), INVALID), ("act -1", dict(act=-1), INVALID),
    ("acc_scale infinite", dict(acc_scale=INF), INVALID), ("bias_scale NaN", dict(bias_scale=NAN), INVALID),
    ("A 8-byte aligned only", dict(A=("+", 8)), INVALID), ("W 8-byte aligned only", dict(W=("+", 8)), INVALID), ("lda % 8", dict(lda=132), INVALID), ("ldw % 8", dict(ldw=140), INVALID),
    ("C 4-byte aligned only", dict(C=("+", 4)), INVALID), ("ldc % 4", dict(ldc=66), INVALID), ("bias 2-byte aligned only", dict(bias=("+", 2)), INVALID),
    ("residual 4-byte aligned only", dict(residual=("+", 4)), INVALID), ("ldr % 4", dict(ldr=70), INVALID), ("rowvec 4-byte aligned only", dict(rowvec=("+", 4)), INVALID),
    ("rowvec_ld % 4", dict(rowvec_ld=66), INVALID),
    ("ln without column sums", {"ln.colsum": 0}, INVALID), ("ln without slots", {"ln.slots": 0}, INVALID), ("ln column sums 8-byte aligned only", {"ln.colsum": ("+", 8)}, INVALID),
    ("ln statistics 4-byte aligned only", {"ln.stats": ("+", 4)}, INVALID), ("stats_out 4-byte aligned only", dict(stats_out=("+", 4)), INVALID),
    ("slabs 8-byte aligned only", dict(splitk=2, partial=("+", 8)), INVALID),
    ("more K slices than k-tiles", dict(splitk=3), SHAPE), ("splitk < 0", dict(splitk=-1), SHAPE), ("splitk 256", dict(K=64 * 256, lda=64 * 256, ldw=64 * 256, splitk=256), SHAPE),
    ("rpb = 65536", dict(rpb=65536, bstride=65536), SHAPE), ("roff = 65536", dict(rpb=4, bstride=81, roff=65536), SHAPE), ("rpb < 0", dict(rpb=-1), SHAPE),
    ("bstride < 0", dict(rpb=4, bstride=-81), SHAPE), ("roff without rpb", dict(roff=5), SHAPE), ("bstride without rpb", dict(bstride=81), SHAPE),
    ("an A of 4 GiB", dict(M=1 << 24), SHAPE), ("a row map that reaches 4 GiB", dict(M=1 << 16, rpb=1, bstride=256), SHAPE), ("a W of 2 GiB", dict(N=1 << 23), SHAPE),
)
CONV_REFUSAL_BASE = dict(B=1, Hs=8, Ws=8, Cin=64, Co=64, stride=1, up=0, pad_lo=1)
CONV_REFUSALS = (
    ("x null", dict(x=0), INVALID), ("Wp null", dict(Wp=0), INVALID), ("y null", dict(y=0), INVALID), ("a K split without slabs", dict(splitk=2, partial=0), INVALID),
    ("Cin % 64", dict(Cin=48), SHAPE), ("Co % 4", dict(Co=62), SHAPE), ("stride 3", dict(stride=3), SHAPE), ("up 2", dict(up=2), SHAPE), ("pad_lo 2", dict(pad_lo=2), SHAPE),
    ("pad_lo -1", dict(pad_lo=-1), SHAPE), ("B < 1", dict(B=0), SHAPE), ("no output pixel", dict(Hs=1, Ws=1, pad_lo=0), SHAPE),
    ("more K slices than k-tiles", dict(splitk=10), SHAPE), ("splitk < 0", dict(splitk=-1), SHAPE),
    ("acc_scale NaN", dict(acc_scale=NAN), INVALID), ("bias_scale infinite", dict(bias_scale=INF), INVALID),
    ("x 8-byte aligned only", dict(x=("+", 8)), INVALID), ("Wp 8-byte aligned only", dict(Wp=("+", 8)), INVALID), ("y 4-byte aligned only", dict(y=("+", 4)), INVALID),
    ("bias 4-byte aligned only", dict(bias=("+", 4)), INVALID), ("rowvec 2-byte aligned only", dict(rowvec=("+", 2)), INVALID),
    ("residual 4-byte aligned only", dict(residual=("+", 4)), INVALID), ("slabs 8-byte aligned only", dict(splitk=2, partial=("+", 8)), INVALID),
)


def refusal_record(kind, ffi, ptr, changes):
    """the ctypes record of a refusal: the base of its kind with `changes` applied. ptr(name) -> the address of a buffer of that name (real on the GPU, never
    dereferenced on the CPU). -> (record, the objects it points to: keep them alive)"""
    import ctypes as C
    keep = []
    if kind == "gemm":
        d = ffi.GemmFormC()
        names = ("A", "W", "bias", "residual", "C", "rowvec", "stats_out", "partial")
        base = GEMM_REFUSAL_BASE
    else:
        d = ffi.ConvFormC()
        names = ("x", "Wp", "bias", "rowvec", "residual", "y", "partial")
        base = CONV_REFUSAL_BASE
    for n in names:
        setattr(d, n, ptr(n))
    for k, v in base.items():
        setattr(d, k, v)
    ln_changes = {k[3:]: v for k, v in changes.items() if k.startswith("ln.")}
    if ln_changes:
        ln = ffi.LnFoldC(ptr("ln.stats"), 1, ptr("ln.colsum"), ptr("ln.fbias"), 1e-5)
        for k, v in ln_changes.items():
            setattr(ln, k, getattr(ln, k) + v[1] if isinstance(v, tuple) else v)
        keep.append(ln)
        d.ln = C.addressof(ln)
    for k, v in changes.items():
        if not k.startswith("ln."):
            setattr(d, k, getattr(d, k) + v[1] if isinstance(v, tuple) else v)
    return d, keep
