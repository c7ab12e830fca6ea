"""fp64 reference of `ia2p_lora_merge` (include/ia2p.h, "LoRA adapters"; kernel: csrc/lora.hip) and the error bound the kernel must meet (None: the exact bits).
Notation of llm_ops_ref.py / unet_ops_ref.py: u = 2^-24 (U), SECOND covers second-order terms, half_ulp16 the fp16 store, `worst` the comparison.

The value, as the header states it and as the kernel source computes it:
    out[i][k] = fp16_rn(s_n),  s_0 = float(base[i][k]),  s_{a+1} = fma(coef[a], acc_a[i][k], s_a),  acc_a = fp32 accumulation of up_a[i][j] down_a[j][k] over j.
The bound, from the operations read in csrc/lora.hip, never from what a kernel returned:
  accumulation   every product of two fp16 values is exact in fp32. They are summed by v_mfma_f32_16x16x32_f16, 32 ranks per step into one accumulator, in an order
                 inside the step that is not known: for ANY order of an fp32 sum of r terms the error is at most (r - 1) u sum_j |up down| to first order. The zero
                 products of the padded rank add nothing. Taken as rank[a] u sum_j |up_a down_a| (SECOND for the higher orders); it reaches the output times |coef[a]|.
  scale-and-add  one fused multiply-add per adapter: one rounding, u on the magnitude it produces, |s_{a+1}| (the exact partial sum plus the error carried so far).
  store          half an fp16 ulp at |ref| + B (with_store16).
  lattice        up, down integers in [-3, 3] times UP_UNIT / DOWN_UNIT, coef a power of two, base a multiple of BASE_UNIT: every product, every partial sum in any order,
                 every scaled sum and every s_a is an integer multiple of one lattice unit below 2^24 of them (`exactness`): fp32 is exact whatever the MFMA does inside,
                 and the only rounding left is the store, which the reference applies (round16). Bound None. |base| reaches 2 while the lattice unit is far below the
                 fp16 spacing there: some outputs need rounding (ties to even among them) and the small ones need none (`rounding_mix`).
"""
import numpy as np
import torch

from llm_ops_ref import SECOND, U, f64, half_ulp16  # noqa: F401
from encoder_ops_ref import round16, with_store16
from unet_ops_ref import LIMIT, gen, ints, worst, accept  # noqa: F401

from instructany2pix_amd.lora import lora_coef

# (N, K, ranks): the issue's table, and one square shape (N == K), the only kind on which swapped factor roles still fit the ABI
CASES = ((1, 8, (1,)), (40, 72, (4,)), (129, 264, (7, 32)), (33, 36, (3,)), (320, 2880, (64,)), (256, 512, (16,) * 8), (48, 48, (5,)))
SQUARE = (48, 48, (5,))
SLICE_CASE, SLICE_ROWS, SLICE_COLS = (129, 264, (7, 32)), (5, 21), (64, 136)          # launch independence: rows 5 .. 20, columns 64 .. 135
UP_UNIT, DOWN_UNIT, BASE_UNIT = 2.0 ** -4, 2.0 ** -5, 2.0 ** -8
WEIGHTS = (0.7, -0.4, 1.0, 0.25, -1.3, 0.55, 2.0, -0.9)          # real-valued cases: adapter a's weight
LATTICE_WEIGHTS = (1.0, -0.5, 0.25, 2.0, -1.0, 0.5, -0.25, 1.0)  # powers of two


def lora_case(N, K, ranks, lattice, seed=None):
    """dict(base [N, K], ups, downs, weights, alphas, ranks, coefs) as fp64 tensors holding fp16 values; coefs = lora_coef(weight, alpha, rank), the fp32 values the ABI gets"""
    g = gen(seed if seed is not None else 1000 * N + K + 7 * len(ranks) + (1 if lattice else 0))
    ups, downs, weights, alphas = [], [], [], []
    for a, r in enumerate(ranks):
        if lattice:
            ups.append(ints((N, r), g) * UP_UNIT)
            downs.append(ints((r, K), g) * DOWN_UNIT)
            weights.append(LATTICE_WEIGHTS[a % 8])
            alphas.append(r / 2.0)                                   # alpha / rank = 1 / 2 exactly, odd ranks included
        else:
            ups.append(round16(torch.randn(N, r, generator=g, dtype=torch.float64) * r ** -0.5))
            downs.append(round16(torch.randn(r, K, generator=g, dtype=torch.float64) * 0.5))
            weights.append(WEIGHTS[a % 8])
            alphas.append(float(r) * (0.5 + 0.25 * (a % 3)))
    if lattice:
        base = torch.randint(-512, 513, (N, K), generator=g).double() * BASE_UNIT      # multiples of 2^-8 in [-2, 2]
        small = torch.rand(N, K, generator=g) < 0.3
        base = torch.where(small, torch.randint(-8, 9, (N, K), generator=g).double() * BASE_UNIT, base)   # ... a third of them near zero: sums that need no rounding
    else:
        base = round16(torch.randn(N, K, generator=g, dtype=torch.float64) * 0.3)
    coefs = [lora_coef(w, al, r) for w, al, r in zip(weights, alphas, ranks)]
    return dict(N=N, K=K, ranks=tuple(ranks), lattice=lattice, base=base, ups=ups, downs=downs, weights=weights, alphas=alphas, coefs=coefs)


def lattice_unit(case):
    return UP_UNIT * DOWN_UNIT * min(abs(c) for c in case["coefs"])


def exactness(case):
    """-> (ok, largest magnitude in lattice units): every operand sits on the lattice and no sum, in any order, leaves the range fp32 holds exactly"""
    unit = lattice_unit(case)
    on = True
    for c in case["coefs"]:
        m, e = np.frexp(abs(c))
        on = on and m == 0.5 and float(np.float32(c)) == c                           # a power of two
    on = on and bool((case["base"] / unit == (case["base"] / unit).round()).all())
    total = case["base"].abs()
    for up, dn, c in zip(case["ups"], case["downs"], case["coefs"]):
        on = on and bool(((up / UP_UNIT).round() == up / UP_UNIT).all()) and bool(((dn / DOWN_UNIT).round() == dn / DOWN_UNIT).all())
        total = total + abs(c) * (up.abs() @ dn.abs())                                # bounds every partial sum of every order, scaled or not
    peak = float(total.max() / unit)
    for up, dn in zip(case["ups"], case["downs"]):
        peak = max(peak, float((up.abs() @ dn.abs()).max() / (UP_UNIT * DOWN_UNIT)))  # the unscaled accumulators, in their own unit
    return on and peak < LIMIT, peak


def rounding_mix(case):
    """(outputs that the fp16 store rounds, outputs it leaves as they are) of a lattice case"""
    s = lora_exact(case)
    moved = round16(s) != s
    return int(moved.sum()), int((~moved).sum())


def lora_exact(case, coefs=None):
    s = case["base"].clone()
    for up, dn, c in zip(case["ups"], case["downs"], case["coefs"] if coefs is None else coefs):
        s = s + float(c) * (up @ dn)
    return s


def lora_ref(case):
    """-> (ref fp64, bound): lattice: (the fp16-rounded exact value, None); real: (the exact value, the bound of the module docstring)"""
    ref = lora_exact(case)
    if case["lattice"]:
        return round16(ref), None
    B = torch.zeros_like(ref)
    s = case["base"].clone()
    for up, dn, c, r in zip(case["ups"], case["downs"], case["coefs"], case["ranks"]):
        B = B + abs(c) * r * U * (up.abs() @ dn.abs())          # the accumulation, whatever its order
        s = s + float(c) * (up @ dn)
        B = B + U * (s.abs() + B)                               # the fused multiply-add's one rounding
    B = B * SECOND
    return ref, with_store16(ref, B)


# ---- a numpy model of the kernel, for the mutants ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("coef_swapped", "last_rank_dropped", "alpha_ignored", "roles_transposed", "rounded_early")


def merge_model(case, mutant=None):
    """The kernel's arithmetic in numpy fp32 (products exact, ranks accumulated in ascending order -- one of the orders the bound covers --, one fused multiply-add per
    adapter, one fp16 rounding), or one of MUTANTS. -> fp64 tensor of fp16 values. A mutant that does not apply to the case returns None."""
    ups = [u.numpy().astype(np.float32) for u in case["ups"]]
    dns = [d.numpy().astype(np.float32) for d in case["downs"]]
    coefs = [np.float32(c) for c in case["coefs"]]
    if mutant == "coef_swapped":
        if len(coefs) < 2 or coefs[0] == coefs[1]:
            return None
        coefs[0], coefs[1] = coefs[1], coefs[0]
    if mutant == "alpha_ignored":
        coefs = [np.float32(w) for w in case["weights"]]
    if mutant == "last_rank_dropped":
        ups, dns = [u[:, :-1] for u in ups], [d[:-1] for d in dns]
    if mutant == "roles_transposed":
        if case["N"] != case["K"]:
            return None
        ups, dns = [d.T.copy() for d in dns], [u.T.copy() for u in ups]
    s = case["base"].numpy().astype(np.float32)
    for up, dn, c in zip(ups, dns, coefs):
        acc = np.zeros_like(s)
        for j in range(up.shape[1]):
            acc = (acc + up[:, j:j + 1] * dn[j:j + 1, :]).astype(np.float32)          # (the product of two fp16 values is exact in fp32)
        if mutant == "rounded_early":
            acc = acc.astype(np.float16).astype(np.float32)
        s = (np.float64(c) * acc.astype(np.float64) + s.astype(np.float64)).astype(np.float32)      # fma: the product is exact in fp64, one rounding that matters
        if mutant == "rounded_early":
            s = s.astype(np.float16).astype(np.float32)
    return torch.from_numpy(s.astype(np.float16).astype(np.float64))
