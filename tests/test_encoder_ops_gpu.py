"""The small launches around the UNet one by one -- CLIP text / prior stem, causal attention and pooling (misc.hip), the VAE's row softmax and 1x1 convolution, the
ViT stem and head projection (vit.hip), the SAM decoder's pieces (sam.hip), the UNet's embeddings, concats and the IP-Adapter attention map -- against the fp64
references of tests/encoder_ops_ref.py.

Every output must lie within the bound encoder_ops_ref derives for its operation from operation counts; pure data movement must be equal to the bit. Every output
buffer starts as fp16 NaN (a sentinel for fp32) with a guard region behind the expected extent that must come back untouched, every output is finite, and a second
launch gives the same bits. Each test prints max(err / bound) before it asserts (pytest -s); docs/LOG.md records a run."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 512
SENTINEL = -7777.0
_INT = {torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}


def _lib():
    from instructany2pix_amd import _ffi
    return _ffi, _ffi.lib()


def _report(tag, worst):
    print(f"[encoder-ops] {tag}: max(err / bound) {worst:.3g}")
    return worst <= 1.0


class Out:
    """an output buffer of n elements: NaN (fp16) or a sentinel (fp32) all over, and GUARD more elements behind the expected extent"""

    def __init__(self, n, dtype=torch.float16, init=None):
        self.n, self.dtype, self.init = int(n), dtype, init
        self.buf = torch.empty(self.n + GUARD, dtype=dtype, device=DEV)
        self.reset()

    def reset(self):
        self.buf.fill_(float("nan") if self.dtype == torch.float16 else SENTINEL)
        if self.init is not None:      # an operation in place: the input
            self.buf[:self.n].copy_(self.init.reshape(-1))
        self.guard0 = self.buf[self.n:].view(_INT[self.dtype]).clone()

    @property
    def out(self):
        return self.buf[:self.n]

    def check(self, tag):
        assert torch.equal(self.buf[self.n:].view(_INT[self.dtype]), self.guard0), f"{tag}: wrote behind its output"
        assert bool(torch.isfinite(self.out.float()).all()), f"{tag}: an output is not finite (or was never written)"


def _twice(tag, launch, outs):
    """launch twice from freshly filled buffers: same bits, guards intact, everything finite. -> the outputs (on the CPU)"""
    bits = []
    for _ in range(2):
        for o in outs:
            o.reset()
        launch()
        torch.cuda.synchronize()
        bits.append([o.buf.view(_INT[o.dtype]).clone() for o in outs])
    for a, b in zip(*bits):
        assert torch.equal(a, b), f"{tag}: a second launch gives other bits"
    for o in outs:
        o.check(tag)
    return [o.out.cpu() for o in outs]


def _ok(st):
    ffi, _ = _lib()
    ffi.check(st)


def _h(t):
    return t.half().to(DEV).contiguous()


def _randh(*shape, seed, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=R.gen(seed))).half()


# ---- causal attention --------------------------------------------------------------------------------------------------------------------------------------
def _attention(qkv, T, heads, tag):
    ffi, lib = _lib()
    d, o = _h(qkv), Out(2 * T * heads * 64)
    return _twice(tag, lambda: _ok(lib.ia2p_causal_attention_small(ffi.current_stream(), ffi.ptr(d), ffi.ptr(o.buf), 2, T, heads, 64)), [o])[0].reshape(2 * T, heads * 64)


@pytest.mark.parametrize("heads", R.ATTN_HEADS)
@pytest.mark.parametrize("T", R.ATTN_T)
def test_causal_attention_small(T, heads):
    """diffuse, planted (a key leading by 20 at 0, 63, 64, q - 1, q: the row is that key's value row) and late-maximum (the largest score in the second key half,
    120 above the first) rows"""
    worst = 0.0
    for fam, T_, heads_, edge in R.attention_cases():
        if (T_, heads_) != (T, heads):
            continue
        tag = f"causal_attention_small T={T} heads={heads} {fam} {edge}"
        qkv = R.attention_case(fam, T, heads, 100 + T, edge)
        ref, bound, _ = R.causal_attention(qkv, 2, T, heads)
        got = _attention(qkv, T, heads, tag)
        worst = max(worst, R.ratio(got, ref, bound))
        if fam == "planted":
            tgt = R.planted_target(T, edge)
            rows = (tgt >= 0).nonzero().flatten()
            if len(rows):
                v = R.f64(qkv).reshape(2, T, 3, heads, 64)[:, :, 2]
                sel = lambda t: t.reshape(2, T, heads, 64)[:, rows]      # noqa: E731
                away = (sel(ref) - v[:, tgt[rows]]).abs()                # what the other keys still weigh (fp64): below 1e-5
                assert float(away.max()) < 1e-5
                assert bool(((sel(got).double() - v[:, tgt[rows]]).abs() <= sel(bound) + away).all()), f"{tag}: a row is not its key's value row"
    assert _report(f"causal_attention_small T={T} heads={heads}", worst)


@pytest.mark.parametrize("T", [2, 64, 65, 77, 127, 128])
def test_causal_attention_never_reads_the_future(T):
    """K and V of every token after p are NaN: rows <= p are finite and have the bits of the clean run"""
    heads = 3
    qkv = R.attention_case("diffuse", T, heads, 7)
    clean = _attention(qkv, T, heads, "clean")
    for p in sorted({0, 63, 64, T - 2} & set(range(T - 1))):
        bad = qkv.clone().reshape(2, T, 3, heads * 64)
        bad[:, p + 1:, 1:] = float("nan")
        ffi, lib = _lib()
        d, o = _h(bad.reshape(2 * T, -1)), torch.full((2 * T, heads * 64), float("nan"), dtype=torch.float16, device=DEV)
        _ok(lib.ia2p_causal_attention_small(ffi.current_stream(), ffi.ptr(d), ffi.ptr(o), 2, T, heads, 64))
        got = o.cpu().reshape(2, T, -1)[:, :p + 1]
        assert bool(torch.isfinite(got.float()).all()), f"T={T} p={p}: a future token leaks"
        assert torch.equal(got.view(torch.int16), clean.reshape(2, T, -1)[:, :p + 1].view(torch.int16)), f"T={T} p={p}"


# ---- CLIP stem and pooling ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 520, 768, 1280])
def test_clip_embed(H):
    ffi, lib = _lib()
    vocab, worst = 50, 0.0
    tok = _randh(vocab, H, seed=H) * torch.linspace(0.25, 4, vocab).half()[:, None]      # rows of differing scales
    for rows, T in [(1, 1), (5, 5), (5, 3), (154, 77), (154, 64)]:
        pos = _randh(T, H, seed=H + T, scale=0.5)
        ids = torch.randint(0, vocab, (rows,), generator=R.gen(rows + T), dtype=torch.int32)
        ids[0] = vocab + 7
        ids[-1] = -3
        if rows > 3:
            ids[1], ids[2] = 0, vocab - 1
        emb = _randh(rows, H, seed=3 * H + rows, scale=2.0)
        # "biased": every entry of embeds is in [1, 2) and pos adds 0.45 fp16 ulp of it, so every store rounds DOWN by that much: statistics summed over the unrounded
        # value are off by 0.45 x 2^-10 per entry, all one way (3.8 to 76 times the bound, H u sum |x|, at these H), where random rounding errors would mostly cancel
        for form in ("ids", "embeds", "biased"):
            tag = f"clip_embed H={H} rows={rows} T={T} {form}"
            e_in, p_in = emb, pos
            if form == "biased":
                e_in = (1 + torch.rand(rows, H, generator=R.gen(H + rows))).half()
                p_in = torch.full((T, H), 0.45 * 2.0 ** -10).half()
            (x, xb), (st, sb) = R.clip_embed(ids, tok, None if form == "ids" else e_in, p_in, rows, T, vocab)
            d_ids, d_tok, d_emb, d_pos = ids.to(DEV), _h(tok), _h(e_in), _h(p_in)
            ox, os_ = Out(rows * H), Out(rows * 2, torch.float32)
            args = (ffi.ptr(d_ids), ffi.ptr(d_tok), None) if form == "ids" else (None, None, ffi.ptr(d_emb))
            gx, gs = _twice(tag, lambda: _ok(lib.ia2p_clip_embed(ffi.current_stream(), *args, ffi.ptr(d_pos), ffi.ptr(ox.buf), ffi.ptr(os_.buf), rows, T, H, vocab)), [ox, os_])
            gx, gs = gx.reshape(rows, H), gs.reshape(rows, 2)
            worst = max(worst, R.ratio(gx, x, xb), R.ratio(gs, st, sb))
            assert torch.equal(gx.double(), R.round16(x)), f"{tag}: not the correctly rounded sum"
            # the statistics are those of the row the kernel stored, to within the summation alone
            own, ownb = R.row_stats(gx.double(), torch.zeros(rows, H, dtype=torch.float64))
            worst = max(worst, R.ratio(gs, own, ownb))
            if form == "biased":
                assert bool((gx.double() < x).all()) and float(((x - gx.double()).sum(-1) / ownb[:, 0]).min()) > 3, tag      # the family does what it says
    assert _report(f"clip_embed H={H}", worst)


@pytest.mark.parametrize("H", [64, 100, 1280])
@pytest.mark.parametrize("T", [1, 20, 64, 65, 77])
def test_clip_pool(T, H):
    """rows of one sequence differ in scale and offset, so a row taken one token early or late cannot pass. Sequences: the winner at 0, 63, 64, T - 1, ties
    64 apart and less (the first wins), the id absent"""
    ffi, lib = _lib()
    worst, EOS = 0.0, 49407
    wins = sorted({0, 63, 64, T - 1} & set(range(T)))
    pairs = [(0, 64), (T - 65, T - 1)] if T >= 65 else []      # two winners 64 apart meet in ONE lane (the in-lane tie-break); the other tie meets across lanes
    nseq = len(wins) + len(pairs) + 2
    x = (torch.randn(nseq, T, H, generator=R.gen(T + H)) * torch.linspace(0.5, 3, T)[None, :, None] + torch.linspace(-1, 1, T)[None, :, None]).half()
    g, b = _randh(H, seed=1, scale=0.2, shift=1.0), _randh(H, seed=2, scale=0.1)
    for eos_id in (2, EOS):
        ids = torch.randint(3, 40000, (nseq, T), generator=R.gen(T), dtype=torch.int32)
        for r, w in enumerate(wins):
            ids[r, w] = EOS
        for r, (lo, hi) in enumerate(pairs):
            ids[len(wins) + r, lo] = ids[len(wins) + r, hi] = EOS
        first = T // 3
        ids[nseq - 2, first] = EOS
        ids[nseq - 2, T - 1] = EOS                   # a tie: `first` wins (T = 1: the same token). The last sequence has no EOS.
        ref, bound, pos = R.clip_pool(ids, x, g, b, eos_id, 1e-5)
        assert pos.tolist()[:nseq - 1] == wins + [lo for lo, _ in pairs] + [first]
        d = [ids.to(DEV), _h(x), _h(g), _h(b)]
        o = Out(ids.shape[0] * H)
        tag = f"clip_pool T={T} H={H} eos={eos_id}"
        got = _twice(tag, lambda: _ok(lib.ia2p_clip_pool(ffi.current_stream(), *[ffi.ptr(t) for t in d], ffi.ptr(o.buf), ids.shape[0], T, H, eos_id, 1e-5)), [o])[0]
        worst = max(worst, R.ratio(got.reshape(-1, H), ref, bound))
    assert _report(f"clip_pool T={T} H={H}", worst)


# ---- VAE ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SOFTMAX_N)
def test_softmax_rows(n):
    ffi, lib = _lib()
    worst = 0.0
    for fam, ld, scale, at in R.softmax_cases(n):
        tag = f"softmax_rows n={n} ld={ld} scale={scale} {fam} {at}"
        x = R.softmax_case(fam, n, ld, n + ld, at)
        ref, bound, _ = R.softmax_rows(x, n, scale)
        o = Out(3 * ld, init=x.to(DEV))
        got = _twice(tag, lambda: _ok(lib.ia2p_softmax_rows(ffi.current_stream(), ffi.ptr(o.buf), ld, 3, n, scale)), [o])[0].reshape(3, ld)
        worst = max(worst, R.ratio(got[:, :n], ref, bound))
        assert torch.equal(got[:, n:], x[:, n:]), f"{tag}: the gap columns changed"
        if fam == "planted" and scale == 1.0:      # e^-30 n is far below an fp16 ulp of 1
            assert got[torch.arange(3), torch.tensor([0, n - 1, at])].tolist() == [1.0] * 3, tag
    assert _report(f"softmax_rows n={n}", worst)


@pytest.mark.parametrize("Ci,Co", [(4, 4), (8, 8), (3, 8), (1, 1)])
def test_conv1x1_nchw(Ci, Co):
    """B HW below the grid cap of 4096 x 256 threads, and above it (the grid-stride loop)"""
    ffi, lib = _lib()
    worst = 0.0
    w, bias = _randh(Co, Ci, seed=Ci), _randh(Co, seed=Co + 1)
    for B, HW in [(1, 1), (3, 1000), (2, 600000)]:
        x = _randh(B, Ci, HW, seed=HW)
        x[..., -1] *= 8                                           # the last pixel of every plane stands out
        ref, bound = R.conv1x1_nchw(x, w, bias)
        d, o = [_h(x), _h(w), _h(bias)], Out(B * Co * HW)
        tag = f"conv1x1_nchw {Ci}->{Co} B={B} HW={HW}"
        got = _twice(tag, lambda: _ok(lib.ia2p_conv1x1_nchw(ffi.current_stream(), *[ffi.ptr(t) for t in d], ffi.ptr(o.buf), B, Ci, Co, HW)), [o])[0]
        worst = max(worst, R.ratio(got.reshape(B, Co, HW), ref, bound))
    assert _report(f"conv1x1_nchw {Ci}->{Co}", worst)


# ---- ViT stem ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,Hi,Wi,ps,stride,pad", [(3, 28, 42, 14, 14, 0), (3, 28, 42, 14, 14, 40), (1, 32, 50, 16, 10, 0), (1, 32, 50, 16, 10, 40), (3, 32, 32, 16, 16, 0),
                                                      (3, 32, 32, 16, 16, 40)])
def test_patch_gather(C_, Hi, Wi, ps, stride, pad):
    ffi, lib = _lib()
    gh, gw, Kpad = (Hi - ps) // stride + 1, (Wi - ps) // stride + 1, C_ * ps * ps + pad
    px = _randh(2, C_, Hi, Wi, seed=Hi + Wi)
    want = R.patch_gather(px, ps, stride, gh, gw, Kpad)
    d, o = _h(px), Out(2 * gh * gw * Kpad)
    got = _twice("patch_gather", lambda: _ok(lib.ia2p_patch_gather(ffi.current_stream(), ffi.ptr(d), ffi.ptr(o.buf), 2, C_, Hi, Wi, ps, stride, gh, gw, Kpad)), [o])[0]
    got = got.reshape(2 * gh * gw, Kpad)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not got[:, C_ * ps * ps:].view(torch.int16).any()      # the pad columns are +0


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [2, 17, 258])
@pytest.mark.parametrize("H", [64, 128, 1280, 2048])
def test_vit_embed(H, T, B):
    """all four presence combinations of the stem and pre LayerNorms, rows of ordinary scale and rows with mean = 50 std; x and the per-row statistics"""
    ffi, lib = _lib()
    worst = 0.0
    g = R.gen(H + T + B)
    cls, pos = torch.randn(H, generator=g).half() * 3, (0.5 * torch.randn(T, H, generator=g)).half()
    sg, sb, pg, pb = [(s + 0.2 * torch.randn(H, generator=g)).half() for s in (1, 0, 1, 0)]
    for family in ("plain", "offset"):
        patches = torch.randn(B * (T - 1), H, generator=g) * torch.linspace(0.5, 2, B * (T - 1))[:, None]
        if family == "offset":
            patches = 0.25 * patches + 12.5 * torch.linspace(0.5, 2, B * (T - 1))[:, None]      # mean = 50 std
        patches = patches.half()
        for stem, pre in [(0, 0), (1, 0), (0, 1), (1, 1)]:
            w = [sg if stem else None, sb if stem else None, pg if pre else None, pb if pre else None]
            (x, xb), (st, stb) = R.vit_embed(patches, cls, pos, *w, 1e-6, B, T)
            d = [_h(patches), _h(cls), _h(pos)] + [None if t is None else _h(t) for t in w]
            ox, os_ = Out(B * T * H), Out(B * T * 2, torch.float32)
            tag = f"vit_embed H={H} T={T} B={B} {family} stem={stem} pre={pre}"
            gx, gs = _twice(tag, lambda: _ok(lib.ia2p_vit_embed(ffi.current_stream(), *[ffi.ptr(t) for t in d], ffi.ptr(ox.buf), ffi.ptr(os_.buf), B, T, H, 1e-6)), [ox, os_])
            gx, gs = gx.reshape(B * T, H), gs.reshape(B * T, 2)
            worst = max(worst, R.ratio(gx, x, xb), R.ratio(gs, st, stb))
            if not pre:      # the cls row skips the stem norm: it is cls + pos[0], correctly rounded
                assert torch.equal(gx[::T].double(), R.round16(cls.double() + pos[0].double()).expand(B, H)), f"{tag}: the cls row"
            # the statistics are those of the row the kernel stored, to within the summation alone
            own, ownb = R.row_stats(gx.double(), torch.zeros(B * T, H, dtype=torch.float64))
            worst = max(worst, R.ratio(gs, own, ownb))
    assert _report(f"vit_embed H={H} T={T} B={B}", worst)


@pytest.mark.parametrize("K", [8, 512, 520, 1280])
def test_vit_project(K):
    ffi, lib = _lib()
    worst = 0.0
    for N in (1, 5, 1024):
        for B in (1, 3):
            X, W = _randh(B, K, seed=K + B, scale=2.0), _randh(N, K, seed=N + K) * torch.linspace(0.5, 2, N).half()[:, None]
            ref, bound = R.vit_project(X, W)
            d, o = [_h(X), _h(W)], Out(B * N, torch.float32)
            got = _twice(f"vit_project K={K} N={N} B={B}", lambda: _ok(lib.ia2p_vit_project(ffi.current_stream(), ffi.ptr(d[0]), ffi.ptr(d[1]), ffi.ptr(o.buf), B, N, K)), [o])[0]
            worst = max(worst, R.ratio(got.reshape(B, N), ref, bound))
    assert _report(f"vit_project K={K}", worst)


# ---- SAM decoder -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hs,Ws,Co", [(1, 1, 1, 8), (2, 5, 7, 16), (1, 20, 20, 64)])
def test_pixel_shuffle2(B, Hs, Ws, Co):
    ffi, lib = _lib()
    g = _randh(B * Hs * Ws, 4 * Co, seed=Hs + Co)
    d, o = _h(g), Out(B * 4 * Hs * Ws * Co)
    got = _twice("pixel_shuffle2", lambda: _ok(lib.ia2p_pixel_shuffle2(ffi.current_stream(), ffi.ptr(d), ffi.ptr(o.buf), B, Hs, Ws, Co)), [o])[0]
    assert torch.equal(got.reshape(B, 2 * Hs, 2 * Ws, Co).view(torch.int16), R.pixel_shuffle2(g, B, Hs, Ws, Co).contiguous().view(torch.int16))


@pytest.mark.parametrize("C_", [8, 32, 512])
def test_hyper_dot(C_):
    ffi, lib = _lib()
    worst = 0.0
    for P in (1, 255, 256, 257, 6400):
        for n in (1, 3):
            stride = C_ + 24
            hyper = _randh(n, stride, seed=P + n)
            up = _randh(n, P, C_, seed=C_ + P) * torch.linspace(0.5, 2, P).half()[None, :, None]
            ref, bound = R.hyper_dot(hyper[:, :C_], up)
            d, o = [_h(hyper), _h(up)], Out(n * P, torch.float32)
            got = _twice(f"hyper_dot C={C_} P={P} n={n}", lambda: _ok(lib.ia2p_hyper_dot(ffi.current_stream(), ffi.ptr(d[0]), stride, ffi.ptr(d[1]), ffi.ptr(o.buf), n, P, C_)), [o])[0]
            worst = max(worst, R.ratio(got.reshape(n, P), ref, bound))
    assert _report(f"hyper_dot C={C_}", worst)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_sam_act(n):
    """ReLU to the bit; GELU against erf in fp64, over every fp16 value in [-8, 8] once (n = 70001 holds them all)"""
    ffi, lib = _lib()
    every = R.all_fp16(-8, 8)
    x = torch.cat([every, _randh(max(n - every.numel(), 0), seed=n, scale=3.0)])[-n:] if n > every.numel() else every[torch.randperm(every.numel(), generator=R.gen(n))[:n]]
    assert n < 70001 or x.numel() == n and every.numel() == 36866
    o = Out(n, init=x.to(DEV))
    relu = _twice(f"sam_act n={n} relu", lambda: _ok(lib.ia2p_sam_act(ffi.current_stream(), ffi.ptr(o.buf), n, 0)), [o])[0]
    assert torch.equal(relu, torch.relu(x.float()).half())
    gelu = _twice(f"sam_act n={n} gelu", lambda: _ok(lib.ia2p_sam_act(ffi.current_stream(), ffi.ptr(o.buf), n, 1)), [o])[0]
    ref, bound = R.gelu(x)
    assert _report(f"sam_act n={n} gelu", R.ratio(gelu, ref, bound))


@pytest.mark.parametrize("n,period", [(8, 8), (2048, 8), (4096, 1024), (24, 24)])
def test_sam_add_rows(n, period):
    """the correctly rounded fp16 sum, into a buffer of its own and into `a` itself"""
    ffi, lib = _lib()
    a, b = _randh(n, seed=n, scale=4.0), _randh(period, seed=period + 1) * torch.linspace(2.0 ** -8, 4, period).half()
    ref, bound, _ = R.add16(a, b.repeat(n // period))
    da, db, o = _h(a), _h(b), Out(n)
    got = _twice("sam_add_rows", lambda: _ok(lib.ia2p_sam_add_rows(ffi.current_stream(), ffi.ptr(da), ffi.ptr(db), ffi.ptr(o.buf), n, period)), [o])[0]
    alias = Out(n, init=da)
    got2 = _twice("sam_add_rows in place", lambda: _ok(lib.ia2p_sam_add_rows(ffi.current_stream(), ffi.ptr(alias.buf), ffi.ptr(db), ffi.ptr(alias.buf), n, period)), [alias])[0]
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16))
    assert torch.equal(got.double(), R.round16(ref)), "not the correctly rounded fp16 sum"
    assert _report(f"sam_add_rows n={n} period={period}", R.ratio(got, ref, bound))


@pytest.mark.parametrize("n,ld", [(1, 1), (1, 4), (300, 1), (300, 4)])
def test_sam_take_col(n, ld):
    ffi, lib = _lib()
    src = _randh(n, ld, seed=n + ld)
    d, o = _h(src), Out(n, torch.float32)
    got = _twice("sam_take_col", lambda: _ok(lib.ia2p_sam_take_col(ffi.current_stream(), ffi.ptr(d), ld, ffi.ptr(o.buf), n)), [o])[0]
    assert torch.equal(got, src[:, 0].float())


# ---- the UNet's embeddings, concats, attention map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Tp,P,Ad,nids", [(320, 1280, 256, 6), (32, 16, 8, 2), (320, 0, 256, 6)])
def test_embed(Tp, P, Ad, nids, B):
    """against fp64, and against diffusers' formula evaluated by torch in fp32 (the sum of the two bounds)"""
    ffi, lib = _lib()
    worst = worst32 = 0.0
    T_VALUES = [0.0, 1.0, 500.5, 999.0]
    ids = torch.tensor([0, 1, 1024, 2047])[torch.randint(0, 4, (B, nids), generator=R.gen(B + nids))].half()
    ids[0, :min(nids, 4)] = torch.tensor([0, 1, 1024, 2047])[:min(nids, 4)].half()
    text = _randh(B, P, seed=P) if P else None
    for ts in [[t] * B for t in T_VALUES] + [[T_VALUES[(b + 1) % 4] for b in range(B)]]:
        for per_batch in (False, True):
            if not per_batch and len(set(ts)) > 1:
                continue
            tsv = torch.tensor(ts, dtype=torch.float32)
            (tref, tb), (aref, ab) = R.embed(tsv, text, ids, Tp, Ad)
            d_ts, d_text, d_ids = tsv.to(DEV), None if text is None else _h(text), _h(ids)
            o1, o2 = Out(B * Tp), Out(B * (P + nids * Ad))
            tag = f"embed Tp={Tp} P={P} Ad={Ad} B={B} t={ts} ts={per_batch}"
            g1, g2 = _twice(tag, lambda: _ok(lib.ia2p_embed(ffi.current_stream(), -1.0 if per_batch else ts[0], ffi.ptr(d_ts) if per_batch else None, ffi.ptr(d_text), ffi.ptr(d_ids),
                                                             ffi.ptr(o1.buf), ffi.ptr(o2.buf), B, Tp, P, Ad, nids)), [o1, o2])
            g1, g2 = g1.reshape(B, Tp), g2.reshape(B, -1)
            worst = max(worst, R.ratio(g1, tref, R.with_store16(tref, tb)), R.ratio(g2, aref, R.with_store16(aref, ab)))
            if P:
                assert torch.equal(g2[:, :P].view(torch.int16), text.view(torch.int16)), f"{tag}: the text columns are a copy"
            t32 = R.sinusoid_diffusers(tsv, Tp).double()
            a32 = R.sinusoid_diffusers(ids.float().reshape(-1), Ad).double().reshape(B, -1)
            worst32 = max(worst32, R.ratio(g1, t32, R.with_store16(t32, tb) + tb), R.ratio(g2[:, P:], a32, R.with_store16(a32, ab[:, P:]) + ab[:, P:]))
    assert _report(f"embed Tp={Tp} P={P} Ad={Ad} B={B} against diffusers' fp32 formula", worst32)
    assert _report(f"embed Tp={Tp} P={P} Ad={Ad} B={B}", worst)


CONCAT_SHAPES = [(Ca, Cb, M) for Ca, Cb in [(8, 8), (320, 640), (1280, 1280)] for M in (1, 257)]


def _concat_all(check):
    """every concat case -> the outputs (CPU). The sources' rows are 16 and 8 elements apart from dense (lda > Ca, ldb > Cb)."""
    ffi, lib = _lib()
    outs = []
    for Ca, Cb, M in CONCAT_SHAPES:
        a, b = _randh(M, Ca + 16, seed=Ca + M), _randh(M, Cb + 8, seed=Cb + M + 1)
        da, db, o = _h(a), _h(b), Out(M * (Ca + Cb))
        launch = lambda: _ok(lib.ia2p_concat(ffi.current_stream(), ffi.ptr(da), Ca + 16, Ca, ffi.ptr(db), Cb + 8, Cb, ffi.ptr(o.buf), M))      # noqa: E731
        if check:
            got = _twice(f"concat {Ca}+{Cb} M={M}", launch, [o])[0].reshape(M, Ca + Cb)
            assert torch.equal(got.view(torch.int16), torch.cat([a[:, :Ca], b[:, :Cb]], 1).view(torch.int16)), (Ca, Cb, M)
        else:
            launch()
            torch.cuda.synchronize()
            got = o.out.cpu().reshape(M, Ca + Cb)
        outs.append(got)
    return outs


def test_concat_both_store_forms(tmp_path):
    """the write-through form (the default of IA2P_WT, read once per process) here, the plain stores in a child process with IA2P_WT=0: the same bits"""
    mine = _concat_all(True)
    path = str(tmp_path / "concat_plain.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--concat-child", path], env=dict(os.environ, IA2P_WT="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    theirs = torch.load(path)
    assert len(theirs) == len(mine)
    for (Ca, Cb, M), x, y in zip(CONCAT_SHAPES, mine, theirs):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f"concat {Ca}+{Cb} M={M}: the two store forms differ"


@pytest.mark.parametrize("Ka,Kb,rows", [(8, 8, 1), (576, 64, 70), (2880, 640, 320)])
def test_cat_rows(Ka, Kb, rows):
    ffi, lib = _lib()
    a, b = _randh(rows, Ka, seed=Ka), _randh(rows, Kb, seed=Kb + 1)
    ba, bb = _randh(rows, seed=rows, scale=2.0), _randh(rows, seed=rows + 1) * torch.linspace(2.0 ** -8, 2, rows).half()
    d = [_h(a), _h(b), _h(ba), _h(bb)]
    o, ob = Out(rows * (Ka + Kb)), Out(rows)
    got, gb = _twice("cat_rows", lambda: _ok(lib.ia2p_cat_rows(ffi.current_stream(), ffi.ptr(d[0]), Ka, ffi.ptr(d[1]), Kb, ffi.ptr(d[2]), ffi.ptr(d[3]), ffi.ptr(o.buf), ffi.ptr(ob.buf), rows)),
                     [o, ob])
    assert torch.equal(got.reshape(rows, Ka + Kb).view(torch.int16), torch.cat([a, b], 1).view(torch.int16))
    ref, bound, _ = R.add16(ba, bb)
    assert _report(f"cat_rows {Ka}+{Kb} rows={rows} bias", R.ratio(gb, ref, bound))


@pytest.mark.parametrize("heads", R.IPMAP_HEADS)
@pytest.mark.parametrize("ntok", R.IPMAP_NTOK)
def test_ip_attn_map(ntok, heads):
    """ldq and ldk larger than heads 64; diffuse K_ip and planted columns (the token softmax is one-hot: an output is the sum of the queries' entries its token leads)"""
    ffi, lib = _lib()
    worst = 0.0
    for fam, ntok_, Nq, heads_ in R.ip_map_cases():
        if (ntok_, heads_) != (ntok, heads):
            continue
        Q, K = R.ip_map_case(fam, ntok, Nq, heads, ntok + Nq)
        ref, bound, _ = R.ip_attn_map(Q, K, heads)
        d, o = [_h(Q), _h(K)], Out(2 * heads * Nq * ntok)
        tag = f"ip_attn_map ntok={ntok} Nq={Nq} heads={heads} {fam}"
        got = _twice(tag, lambda: _ok(lib.ia2p_ip_attn_map(ffi.current_stream(), ffi.ptr(d[0]), Q.shape[-1], ffi.ptr(d[1]), K.shape[-1], ffi.ptr(o.buf), 2, heads, Nq, ntok)), [o])[0]
        worst = max(worst, R.ratio(got.reshape(2, heads, Nq, ntok), ref, bound))
    assert _report(f"ip_attn_map ntok={ntok} heads={heads}", worst)


if __name__ == "__main__":      # the child of test_concat_both_store_forms
    assert sys.argv[1] == "--concat-child"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.save(_concat_all(False), sys.argv[2])
