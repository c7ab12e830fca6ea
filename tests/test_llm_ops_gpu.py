"""The launches of the LLM decode and prefill paths one by one (ia2p_llm_gemv_epi, _gemv_qkv, _attention_rows, _attention_prefill, _rmsnorm_rows,
_rope_cache_rows, _silu_mul_rows) against the fp64 references of tests/llm_ops_ref.py.

Every output must lie within the bound llm_ops_ref derives for its operation from operation counts (no tolerance is taken from a kernel's output), at the
smallest shapes where these kernels change path: both workgroup forms of the GEMVs and a ragged last workgroup, one row and several, every 16- and 256-key
block edge of the attention up to 8192 keys, cache rows and rotary angles up to position 8191. Each test prints max(err / bound) over its outputs before it
asserts (pytest -s); docs/LOG.md records a run."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = ["fp16", "fp4", "nf4"]
MS = (1, 2, 3, 5, 8)
PLAIN, RESID, SWIGLU = 0, 1, 2
OK, INVALID, SHAPE = 0, 1, 2
EPS = 1e-5
NAN16 = float("nan")


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(K, seed):
    """8 input rows of differing scales (a row taken for another cannot pass)"""
    return (torch.randn(8, K, generator=_gen(seed)) * torch.tensor([1.0, 0.25, 3.0, 0.5, 7.0, 0.125, 2.0, 11.0])[:, None]).to(DEV).contiguous()


def _gamma(K, seed):
    return (1.0 + 0.25 * torch.randn(K, generator=_gen(seed))).half().to(DEV)


class Weights:
    """a [N, K] projection in one weight format: the arguments the entry points take, and the exact matrix the kernel multiplies by (fp64)"""

    def __init__(self, fmt, N, K, seed, w=None):
        from instructany2pix_amd.config import BNB_4BIT_CODEBOOKS
        ffi, lib = _lib()
        self.N, self.K = N, K
        w = ((torch.randn(N, K, generator=_gen(seed)) * K ** -0.5) if w is None else w).half().to(DEV)
        if fmt == "fp16":
            self.W, self.absmax, self.cb, self.exact = w, None, None, w.cpu().double()
            return
        self.cb = (C.c_float * 16)(*BNB_4BIT_CODEBOOKS[fmt])
        self.W = torch.empty(lib.ia2p_llm_q4_packed_bytes(N, K), dtype=torch.uint8, device=DEV)
        self.absmax = torch.empty(N * K // 64, dtype=torch.float32, device=DEV)
        ffi.check(lib.ia2p_llm_quantize_q4(ffi.current_stream(), ffi.ptr(w), N, K, self.cb, ffi.ptr(self.W), ffi.ptr(self.absmax)), None, llm=True)
        self.exact = R.unpack_q4(self.W, self.absmax, BNB_4BIT_CODEBOOKS[fmt], N, K)

    def args(self):
        ffi, _ = _lib()
        return ffi.ptr(self.W), ffi.ptr(self.absmax), self.cb


def _gemv_epi(wt, x, epi, out, gamma=None, hid=None):
    ffi, lib = _lib()
    st = lib.ia2p_llm_gemv_epi(ffi.current_stream(), *wt.args(), ffi.ptr(x), ffi.ptr(gamma), EPS, epi, ffi.ptr(out), ffi.ptr(hid), wt.N, wt.K, x.shape[0])
    ffi.check(st, None, llm=True)


def _report(tag, worst):
    print(f"[llm-ops] {tag}: max(err / bound) {worst:.3g}")
    return worst <= 1.0


# ---- the GEMVs with an epilogue --------------------------------------------------------------------------------------------------------------------------
def _gemv_shapes(fmt, case):
    Ks = [8, 64, 512, 1408, 2056] if fmt == "fp16" else [64, 512, 1408]
    Ns = [2 * 66, 2 * 1408, 2 * 4097] if case == "swiglu" else [517, 8200]
    return [(N, K) for K in Ks for N in Ns]


@pytest.mark.parametrize("case", ["resid", "swiglu", "plain_gamma", "plain"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_gemv_epilogues(fmt, case):
    """residual (from a non-zero out, no gamma: o_proj, down_proj), SwiGLU (with gamma: gate / up), plain with gamma and hid (lm_head), plain. Row m of the
    one-row launch against fp64; every M-row launch equal to the one-row launches bit for bit."""
    epi = {"resid": RESID, "swiglu": SWIGLU}.get(case, PLAIN)
    worst = 0.0
    for N, K in _gemv_shapes(fmt, case):
        wt, x = Weights(fmt, N, K, 3 + N + K), _rows(K, N + 7 * K)
        gamma = _gamma(K, K + 1) if case in ("swiglu", "plain_gamma") else None
        n_out = N // 2 if case == "swiglu" else N
        out0 = torch.randn(8, n_out, generator=_gen(N)).to(DEV) if case == "resid" else torch.full((8, n_out), NAN16, device=DEV)
        hid_ref = None
        if case == "resid":
            ref, bound = R.gemv_resid(wt.exact, x, out0)
        elif case == "swiglu":
            ref, bound = R.gemv_swiglu(wt.exact, x, gamma, EPS)
        else:
            ref, bound, hid_ref, hid_bound = R.gemv_plain(wt.exact, x, gamma, EPS)

        def launch(lo, M):
            out = out0[lo:lo + M].clone()
            hid = torch.full((M, K), NAN16, device=DEV) if hid_ref is not None else None
            _gemv_epi(wt, x[lo:lo + M], epi, out, gamma, hid)
            return out, hid

        single = [launch(m, 1) for m in range(8)]
        out1 = torch.cat([o for o, _ in single])
        worst = max(worst, R.ratio(out1, ref, bound))
        if hid_ref is not None:
            hid1 = torch.cat([h for _, h in single])
            worst = max(worst, R.ratio(hid1, hid_ref, hid_bound))
        for M in MS[1:]:
            out, hid = launch(0, M)
            assert torch.equal(out, out1[:M]), f"{fmt} {case} {N} x {K}, M = {M}: rows differ from the one-row launches"
            assert hid is None or torch.equal(hid, hid1[:M]), f"{fmt} {case} {N} x {K}, M = {M}: hid rows differ from the one-row launches"
    assert _report(f"gemv {case} {fmt}", worst)


# ---- QKV GEMV + RoPE + cache write, and the prefill row kernel ---------------------------------------------------------------------------------------------
QKV_POS = [0, 1, 255, 256, 4095, 8191, 1, 255]          # one M = 8 launch, every row in its own caches


def _pattern(rows, H, salt):
    """a cache of finite fp16 bit patterns (compared as int16)"""
    n = rows * H
    return ((torch.arange(n, device=DEV, dtype=torch.int64) * 7 + salt) % 30011 + 1).to(torch.int16).view(torch.float16).reshape(rows, H)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inv_freq(theta=10000.0):
    _, lib = _lib()
    f = (C.c_float * 64)()
    assert lib.ia2p_llm_rope_inv_freq(theta, f) == OK
    return torch.tensor(list(f), dtype=torch.float32).to(DEV)


def _gemv_qkv(wt, x, gamma, inv_freq, pos, q, kcs, vcs, H):
    ffi, lib = _lib()
    M = x.shape[0]
    st = lib.ia2p_llm_gemv_qkv(ffi.current_stream(), *wt.args(), ffi.ptr(x), ffi.ptr(gamma), EPS, ffi.ptr(inv_freq), (C.c_int32 * M)(*pos), ffi.ptr(q),
                               (C.c_void_p * M)(*[t.data_ptr() for t in kcs]), (C.c_void_p * M)(*[t.data_ptr() for t in vcs]), H, wt.K, M)
    ffi.check(st, None, llm=True)


def _others_untouched(after, before, rows):
    keep = torch.ones(before.shape[0], dtype=torch.bool, device=DEV)
    keep[list(rows)] = False
    return torch.equal(_bits(after)[keep], _bits(before)[keep])


@pytest.mark.parametrize("H", [128, 384, 2816])
@pytest.mark.parametrize("fmt", FORMATS)
def test_gemv_qkv_rope_and_cache_write(fmt, H):
    K = 512 if H < 2816 else 192
    wt, x, gamma, inv_freq = Weights(fmt, 3 * H, K, 5 + H), _rows(K, H + 11), _gamma(K, H + 3), _inv_freq()
    ref = R.gemv_qkv(wt.exact, x, QKV_POS, inv_freq, gamma, EPS)
    before = [(_pattern(p + 2, H, 2 * m), _pattern(p + 2, H, 2 * m + 1)) for m, p in enumerate(QKV_POS)]
    kcs, vcs = [b[0].clone() for b in before], [b[1].clone() for b in before]
    q = torch.full((8, H), NAN16, device=DEV)
    _gemv_qkv(wt, x, gamma, inv_freq, QKV_POS, q, kcs, vcs, H)
    torch.cuda.synchronize()
    k_rows, v_rows = torch.stack([kcs[m][p] for m, p in enumerate(QKV_POS)]), torch.stack([vcs[m][p] for m, p in enumerate(QKV_POS)])
    worst = max(R.ratio(q, *ref["q"]), R.ratio(k_rows, *ref["k"]), R.ratio(v_rows, *ref["v"]))
    for m, p in enumerate(QKV_POS):
        assert _others_untouched(kcs[m], before[m][0], [p]) and _others_untouched(vcs[m], before[m][1], [p]), f"row {m}: a cache row other than {p} was written"
    for M in MS:                       # the first M rows again (M = 1: every row alone), into restored cache rows: the same bits
        for lo in (range(8) if M == 1 else [0]):
            for m in range(lo, lo + M):
                kcs[m][QKV_POS[m]], vcs[m][QKV_POS[m]] = before[m][0][QKV_POS[m]], before[m][1][QKV_POS[m]]
            q2 = torch.full((M, H), NAN16, device=DEV)
            _gemv_qkv(wt, x[lo:lo + M], gamma, inv_freq, QKV_POS[lo:lo + M], q2, kcs[lo:lo + M], vcs[lo:lo + M], H)
            assert torch.equal(q2, q[lo:lo + M]), f"M = {M} from row {lo}: q rows differ"
            for m in range(lo, lo + M):
                assert torch.equal(_bits(kcs[m][QKV_POS[m]]), _bits(k_rows[m])) and torch.equal(_bits(vcs[m][QKV_POS[m]]), _bits(v_rows[m])), f"M = {M}: cache row of row {m} differs"
    assert _report(f"qkv + rope + cache {fmt} H={H}", worst)


def _rope_cache_rows(qkv, inv_freq, q, kc, vc, H, p0):
    ffi, lib = _lib()
    st = lib.ia2p_llm_rope_cache_rows(ffi.current_stream(), ffi.ptr(qkv), ffi.ptr(inv_freq), ffi.ptr(q), ffi.ptr(kc), ffi.ptr(vc), H, p0, qkv.shape[0])
    ffi.check(st, None, llm=True)


@pytest.mark.parametrize("p0", [0, 250, 8188])
@pytest.mark.parametrize("H", [128, 384, 2816])
def test_rope_cache_rows(H, p0):
    T, inv_freq = 4, _inv_freq()
    qkv = (torch.randn(T, 3 * H, generator=_gen(H + p0)) * 2).half().to(DEV)
    ref = R.rope_rows(qkv, p0, inv_freq)
    k0, v0 = _pattern(p0 + T + 1, H, 1), _pattern(p0 + T + 1, H, 2)
    kc, vc, q = k0.clone(), v0.clone(), torch.full((T, H), NAN16, device=DEV)
    _rope_cache_rows(qkv, inv_freq, q, kc, vc, H, p0)
    torch.cuda.synchronize()
    worst = max(R.ratio(q, *ref["q"]), R.ratio(kc[p0:p0 + T], *ref["k"]))
    assert torch.equal(_bits(vc[p0:p0 + T]), _bits(qkv[:, 2 * H:])), "a v-cache row is a copy of the v columns"
    assert _others_untouched(kc, k0, range(p0, p0 + T)) and _others_untouched(vc, v0, range(p0, p0 + T))
    assert _report(f"rope + cache rows H={H} p0={p0}", worst)


def test_decode_row_and_prefill_row_agree_on_equal_inputs():
    """Small-integer weights and inputs: the 3 H sums are exact in fp32 and in fp16, so the QKV GEMV rotates the very values the prefill kernel reads from
    its fp16 qkv row. The two may differ by the sum of their bounds (each is the rotated-pair term, plus the fp16 rounding for k); v is equal bit for bit."""
    H, K, inv_freq = 256, 64, _inv_freq()
    w = torch.randint(-2, 3, (3 * H, K), generator=_gen(1)).float()
    x = torch.randint(-3, 4, (8, K), generator=_gen(2)).float().to(DEV)
    wt = Weights("fp16", 3 * H, K, 0, w=w)
    qkv = (x.cpu().double() @ w.double().t())
    assert float(qkv.abs().max()) <= 2048 and torch.equal(qkv.half().double(), qkv)
    qkv = qkv.half().to(DEV)
    kcs, vcs = [torch.zeros(p + 1, H, dtype=torch.float16, device=DEV) for p in QKV_POS], [torch.zeros(p + 1, H, dtype=torch.float16, device=DEV) for p in QKV_POS]
    qd = torch.full((8, H), NAN16, device=DEV)
    _gemv_qkv(wt, x, None, inv_freq, QKV_POS, qd, kcs, vcs, H)
    dec = R.gemv_qkv(wt.exact, x, QKV_POS, inv_freq)
    worst = 0.0
    for m, p in enumerate(QKV_POS):
        kc, vc = torch.zeros(p + 1, H, dtype=torch.float16, device=DEV), torch.zeros(p + 1, H, dtype=torch.float16, device=DEV)
        qp = torch.full((1, H), NAN16, device=DEV)
        _rope_cache_rows(qkv[m:m + 1], inv_freq, qp, kc, vc, H, p)
        pre = R.rope_rows(qkv[m:m + 1], p, inv_freq)
        worst = max(worst, R.ratio(qd[m:m + 1], qp, dec["q"][1][m:m + 1] + pre["q"][1]), R.ratio(kcs[m][p:p + 1], kc[p:p + 1], dec["k"][1][m:m + 1] + pre["k"][1]))
        assert torch.equal(_bits(vcs[m][p]), _bits(vc[p])) and torch.equal(_bits(vc[p]), _bits(qkv[m, 2 * H:]))
    assert _report("decode row against prefill row", worst)


# ---- attention against the cache -------------------------------------------------------------------------------------------------------------------------
NKS = [1, 2, 3, 5, 15, 16, 17, 255, 256, 257, 511, 513, 1025, 4097, 8192]
PAD = 16                    # rows at and past nk: fp16 NaN (never read)


def _planted_at(nk):
    return sorted({j for j in (0, 15, 16, 255, 256, 257, 511, 512, nk - 17, nk - 16, nk - 1) if 0 <= j < nk})


def _attn_inputs(family, nk, H, seed, rows=None):
    """q [rows or 1, H] fp32 and caches [nk + PAD, H] fp16 (device), the pad rows NaN.
    diffuse: scores ~ N(0, 1/16), near-uniform weights. planted: the keys at the block edges score 22 (big: 100), the others ~ N(0, 1/4) (big: -100 + that).
    big_late: as big, planted from key 256 on only, so the maximum lies behind the first 256 keys and nothing before it comes within 88 of it."""
    g, h, T = _gen(seed), H // 128, rows or 1
    q = torch.randn(T, H, generator=g)
    v = torch.randn(nk + PAD, H, generator=g)
    if family == "diffuse":
        k = 0.25 * torch.randn(nk + PAD, H, generator=g)
    else:
        top = 22.0 if family == "planted" else 100.0
        q[1:] = q[0] + 0.05 * q[1:]                  # several query rows: all near the planted direction
        q0 = q[0].reshape(h, 128)
        unit = q0 / (R.ATTN_SCALE * (q0 * q0).sum(1, keepdim=True))          # scale q . unit = 1 per head
        k = 0.5 * torch.randn(nk + PAD, H, generator=g)
        if family != "planted":
            k = k - top * unit.reshape(1, H)
        k[[j for j in _planted_at(nk) if j >= 256 or family != "big_late"]] = top * unit.reshape(1, H)
    k[nk:], v[nk:] = NAN16, NAN16
    return q.to(DEV), k.half().to(DEV), v.half().to(DEV)


def _attention_rows(q, kcs, vcs, pos, H):
    ffi, lib = _lib()
    M = q.shape[0]
    out = torch.full((M, H), NAN16, device=DEV)
    st = lib.ia2p_llm_attention_rows(ffi.current_stream(), ffi.ptr(q), (C.c_void_p * M)(*[t.data_ptr() for t in kcs]), (C.c_void_p * M)(*[t.data_ptr() for t in vcs]),
                                     (C.c_int32 * M)(*pos), ffi.ptr(out), H // 128, H, M)
    ffi.check(st, None, llm=True)
    return out


def _attention_prefill(q, kc, vc, p0, H):
    ffi, lib = _lib()
    out = torch.full((q.shape[0], H), NAN16, dtype=torch.float16, device=DEV)
    ffi.check(lib.ia2p_llm_attention_prefill(ffi.current_stream(), ffi.ptr(q), ffi.ptr(kc), ffi.ptr(vc), ffi.ptr(out), H // 128, H, p0, q.shape[0]), None, llm=True)
    return out


@pytest.mark.parametrize("H", [128, 384])
@pytest.mark.parametrize("nk", NKS)
def test_attention_one_row(nk, H):
    """both forms (a decoded row: fp32 out; a prefill row at p0 = nk - 1: fp16 out) on the diffuse (nk <= 513) and the planted family; at nk = 257 also planted
    scores of +100 over a background of -100, and at nk = 257 and 513 the same with no planted key among the first 256 (a maximum taken over the first 256 keys
    only would leave e^200)"""
    worst = 0.0
    for family in (["diffuse"] if nk <= 513 else []) + ["planted"] + (["big"] if nk == 257 else []) + (["big_late"] if nk in (257, 513) else []):
        q, kc, vc = _attn_inputs(family, nk, H, 13 * nk + H)
        ref32, ref16 = R.attention_row(q[0], kc[:nk], vc[:nk]), R.attention_row(q[0], kc[:nk], vc[:nk], fp16_out=True)
        dec, pre = _attention_rows(q, [kc], [vc], [nk - 1], H), _attention_prefill(q, kc, vc, nk - 1, H)
        assert torch.equal(dec, _attention_rows(q, [kc], [vc], [nk - 1], H)) and torch.equal(pre, _attention_prefill(q, kc, vc, nk - 1, H)), "two launches differ"
        r = max(R.ratio(dec[0], *ref32), R.ratio(pre[0], *ref16))
        print(f"[llm-ops] attention nk={nk} H={H} {family}: max(err / bound) {r:.3g}")
        worst = max(worst, r)
    assert worst <= 1.0


ATTN_POS = [0, 15, 16, 255, 256, 257, 1000, 8191]


@pytest.mark.parametrize("H", [128, 384])
def test_attention_eight_rows_equal_each_row_alone(H):
    cases = [_attn_inputs("planted", p + 1, H, 31 * p + H) for p in ATTN_POS]
    q, kcs, vcs = torch.cat([c[0] for c in cases]), [c[1] for c in cases], [c[2] for c in cases]
    out = _attention_rows(q, kcs, vcs, ATTN_POS, H)
    assert torch.equal(out, _attention_rows(q, kcs, vcs, ATTN_POS, H)), "two launches differ"
    worst = 0.0
    for m, p in enumerate(ATTN_POS):
        assert torch.equal(out[m:m + 1], _attention_rows(q[m:m + 1], kcs[m:m + 1], vcs[m:m + 1], [p], H)), f"row {m} (position {p}) differs from the row alone"
        worst = max(worst, R.ratio(out[m], *R.attention_row(q[m], kcs[m][:p + 1], vcs[m][:p + 1])))
    assert _report(f"attention 8 rows H={H}", worst)


@pytest.mark.parametrize("H", [128, 384])
@pytest.mark.parametrize("p0,T,family,check", [(254, 5, "diffuse", range(5)), (8189, 3, "planted", range(3)), (0, 300, "diffuse", (0, 15, 16, 255, 256, 299))])
def test_attention_prefill_rows(p0, T, family, check, H):
    """T causal rows of one launch: row t sees the keys 0 .. p0 + t and none of the later rows' (those are finite here: reading one would not show as NaN)"""
    q, kc, vc = _attn_inputs(family, p0 + T, H, p0 + T + H, rows=T)
    out = _attention_prefill(q, kc, vc, p0, H)
    assert torch.equal(out, _attention_prefill(q, kc, vc, p0, H)), "two launches differ"
    assert bool(torch.isfinite(out).all())
    worst = max(R.ratio(out[t], *R.attention_row(q[t], kc[:p0 + t + 1], vc[:p0 + t + 1], fp16_out=True)) for t in check)
    assert _report(f"attention prefill p0={p0} T={T} H={H}", worst)


# ---- the other prefill row kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("H", [128, 1408, 4096])
def test_rmsnorm_rows(H, T):
    ffi, lib = _lib()
    g = _gen(H + T)
    x = torch.randn(T, H, generator=g)
    x[(T - 1) // 2] = 200.0 * torch.sign(x[(T - 1) // 2]) * (1 + 0.1 * torch.randn(H, generator=g))          # sum of squares ~ 4e4 H (1.6e8 at H = 4096)
    x, gamma = x.half().to(DEV), _gamma(H, H)
    y = torch.full((T, H), NAN16, dtype=torch.float16, device=DEV)
    ffi.check(lib.ia2p_llm_rmsnorm_rows(ffi.current_stream(), ffi.ptr(x), ffi.ptr(gamma), EPS, ffi.ptr(y), T, H), None, llm=True)
    assert _report(f"rmsnorm rows H={H} T={T}", R.ratio(y, *R.rmsnorm_rows(x, gamma, EPS)))


@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("I", [128, 1408, 4096])
def test_silu_mul_rows(I, T):
    ffi, lib = _lib()
    gu = torch.randn(T, 2 * I, generator=_gen(I + T)) * 3
    gu[:, 0:8] = torch.tensor([20.0, -20.0, 0.0, -0.0, 20.0, -20.0, 0.0, 1.0])
    gu[:, I - 2:I] = torch.tensor([-20.0, 20.0])
    gu = gu.half().to(DEV)
    act = torch.full((T, I), NAN16, dtype=torch.float16, device=DEV)
    ffi.check(lib.ia2p_llm_silu_mul_rows(ffi.current_stream(), ffi.ptr(gu), ffi.ptr(act), T, I), None, llm=True)
    assert _report(f"silu-multiply rows I={I} T={T}", R.ratio(act, *R.silu_mul_rows(gu)))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    ffi, lib = _lib()
    s, H, K = ffi.current_stream(), 128, 64
    wt, x, inv_freq = Weights("fp16", 3 * H, K, 1), _rows(K, 2), _inv_freq()
    out, q = torch.full((8, 3 * H), 7.0, device=DEV), torch.full((8, H), 7.0, device=DEV)
    o16 = torch.full((8, H), 7.0, dtype=torch.float16, device=DEV)
    kc, vc = _pattern(16, H, 1), _pattern(16, H, 2)
    k0, v0 = kc.clone(), vc.clone()
    W, X, one = ffi.ptr(wt.W), ffi.ptr(x), (C.c_void_p * 8)(*[kc.data_ptr()] * 8)
    pos = lambda *p: (C.c_int32 * 8)(*(list(p) + [0] * (8 - len(p))))      # noqa: E731
    calls = [(lib.ia2p_llm_gemv_epi(s, W, None, None, X, None, 0.0, PLAIN, ffi.ptr(out), None, 3 * H, K, 9), SHAPE),
             (lib.ia2p_llm_gemv_epi(s, W, None, None, X, None, 0.0, 3, ffi.ptr(out), None, 3 * H, K, 1), INVALID),
             (lib.ia2p_llm_gemv_epi(s, W, None, None, X, None, 0.0, SWIGLU, ffi.ptr(out), None, 3 * H - 1, K, 1), SHAPE),
             (lib.ia2p_llm_gemv_epi(s, W, None, None, X, None, 0.0, PLAIN, ffi.ptr(out), ffi.ptr(q), 3 * H, K, 1), INVALID),
             (lib.ia2p_llm_gemv_qkv(s, W, None, None, X, None, 0.0, ffi.ptr(inv_freq), pos(3, 8192), ffi.ptr(q), one, one, H, K, 2), SHAPE),
             (lib.ia2p_llm_gemv_qkv(s, W, None, None, X, None, 0.0, ffi.ptr(inv_freq), pos(3, -1), ffi.ptr(q), one, one, H, K, 2), SHAPE),
             (lib.ia2p_llm_gemv_qkv(s, W, None, None, X, None, 0.0, ffi.ptr(inv_freq), pos(3), ffi.ptr(q), one, one, 192, K, 1), SHAPE),
             (lib.ia2p_llm_attention_rows(s, ffi.ptr(q), one, one, pos(3, 8192), ffi.ptr(out), 1, H, 2), SHAPE),
             (lib.ia2p_llm_attention_rows(s, ffi.ptr(q), one, one, pos(3), ffi.ptr(out), 2, H, 1), SHAPE),
             (lib.ia2p_llm_attention_rows(s, ffi.ptr(q), one, one, pos(3), ffi.ptr(out), 1, H, 9), SHAPE),
             (lib.ia2p_llm_attention_prefill(s, ffi.ptr(q), ffi.ptr(kc), ffi.ptr(vc), ffi.ptr(o16), 1, H, 8190, 3), SHAPE),
             (lib.ia2p_llm_attention_prefill(s, ffi.ptr(q), ffi.ptr(kc), ffi.ptr(vc), ffi.ptr(o16), 1, 256, 0, 3), SHAPE),
             (lib.ia2p_llm_rope_cache_rows(s, ffi.ptr(out), ffi.ptr(inv_freq), ffi.ptr(q), ffi.ptr(kc), ffi.ptr(vc), H, 8190, 3), SHAPE),
             (lib.ia2p_llm_rope_cache_rows(s, ffi.ptr(out), ffi.ptr(inv_freq), ffi.ptr(q), ffi.ptr(kc), ffi.ptr(vc), 192, 0, 3), SHAPE),
             (lib.ia2p_llm_rmsnorm_rows(s, ffi.ptr(o16), ffi.ptr(o16), EPS, ffi.ptr(o16), 0, H), SHAPE),
             (lib.ia2p_llm_silu_mul_rows(s, ffi.ptr(o16), ffi.ptr(o16), 1, 0), SHAPE)]
    torch.cuda.synchronize()
    assert [got for got, _ in calls] == [want for _, want in calls]
    assert bool((out == 7).all()) and bool((q == 7).all()) and bool((o16 == 7).all())
    assert torch.equal(_bits(kc), _bits(k0)) and torch.equal(_bits(vc), _bits(v0))
