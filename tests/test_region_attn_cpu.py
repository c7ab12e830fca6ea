"""The reference of tests/region_attn_ref.py against an independent, straightforward restatement in torch float64 (a loop over the groups of plain softmaxes: a wrong
reference cannot bless a wrong kernel); the condition under which the two hardware models may stand in the bound (a tenth each, for every case test_region_attn_gpu.py
launches); faults a rewrite of the kernel could plant, which must leave the bound; the pyramid reference against avg_pool2d; the padding rule and the union mask of
inpaint.py / batch.py on CPU tensors; and the host-side refusals of the two entry points (none reaches a HIP call)."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_attn_ref as R  # noqa: E402
import unet_attn_ref as UA  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _restated(c):
    """the formula, written out: per batch row and head, one softmax over the text keys, then a loop over the groups of four-key softmaxes"""
    _, B, heads, Nq, n0, G, kind, w0 = c
    q, k0, v0, k1, v1, m = R.case(*c)
    sp = lambda t: t.double().reshape(B, -1, heads, 64)      # noqa: E731
    q, k0, v0, k1, v1 = sp(q), sp(k0), sp(v0), sp(k1), sp(v1)
    out = torch.zeros(B, Nq, heads, 64, dtype=torch.float64)
    w0 = float(torch.tensor(w0, dtype=torch.float32))
    for b in range(B):
        s = float(torch.tensor(R.S_B[b], dtype=torch.float32))
        for h in range(heads):
            out[b, :, h] = w0 * torch.softmax(q[b, :, h] @ k0[b, :, h].T / 8.0, -1) @ v0[b, :, h]
            for g in range(G):
                kg, vg = k1[b, 4 * g:4 * g + 4, h], v1[b, 4 * g:4 * g + 4, h]
                out[b, :, h] += s * m[b, g].double().reshape(Nq, 1) * (torch.softmax(q[b, :, h] @ kg.T / 8.0, -1) @ vg)
    return out.reshape(B, Nq, heads * 64)


@pytest.mark.parametrize("c", [("diffuse",) + R.NQ_SWEEP[1], ("peaked",) + R.G_SWEEP[3], ("ramp",) + R.G_SWEEP[4], ("planted",) + R.N0_SWEEP[0], ("diffuse",) + R.MASK_SWEEP[3]], ids=str)
def test_reference_is_a_loop_of_plain_softmaxes(c):
    got, want = R.ref(*c)[0], _restated(c)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_models_keep_to_a_tenth_of_the_bound(shape):
    """`region_attention` asserts it (`_check_shares`); here for every case of the GPU test, with the figures"""
    for family in R.FAMILIES:
        _, bound, (ex, mf) = R.ref(family, *shape)
        print(f"[region-attn] {family} {shape}: exponential {ex:.3f}, MFMA {mf:.3f} of the bound")
        assert ex <= 0.1 and mf <= 0.1 and bool((bound > 0).all())


def test_degenerate_cases_keep_to_a_tenth_too():
    """the two-segment and one-segment references the GPU test borrows from unet_attn_ref at shapes its own lists do not hold"""
    for family in UA.FAMILIES:
        for n0, w0, s in ((77, 1.0, 1.0), (64, 0.5, 1.3), (120, 1.0, 0.7)):
            UA.ref(family, 2, 3, UA.TWO_NQ, n0, 4, w0, s)
        for n0 in (77, 64):
            UA.ref(family, 2, 3, UA.TWO_NQ, n0, 0, 1.0, 0.0)


def test_case_lists_reach_what_they_are_for():
    shapes = R.SHAPES
    assert {s[2] for s in shapes} == {16, 64, 160, 256} and {s[1] for s in shapes} == {2, 5}
    assert {s[3] for s in shapes} == {64, 77, 120, 300} and {s[4] for s in shapes} == {1, 2, 3, 8, 9, 16}
    assert {s[5] for s in shapes} == set(R.MASKS) and len(shapes) < 40
    for kind in R.MASKS:
        m = R.masks(kind, 2, 3, 160)
        assert not torch.equal(m[0], m[1]) and bool(torch.isfinite(m.float()).all())
    assert bool((R.masks("zero", 2, 3, 160)[:, 1] == 0).all()) and bool((R.masks("one", 2, 3, 160)[:, 1] == 1).all())
    assert float(R.masks("big", 2, 3, 160).max()) > 1.25
    r = R.masks("rect", 2, 3, 160)
    assert set(r.unique().tolist()) == {0.0, 1.0} and bool((r.sum(1) == 1).all())      # disjoint, and they cover the grid


# ---- faults the bound must catch ------------------------------------------------------------------------------------------------------------------------------
def _worst(c, out):
    ref, bound, _ = R.ref(*c)
    return float(((out - ref).abs() / bound).max())


def _groups(c, fn):
    """the restated formula with the image-token part replaced by fn(b, h, q_bh, k1_bh, v1_bh, m_b, s_b) -> [Nq, 64]"""
    _, B, heads, Nq, n0, G, kind, w0 = c
    q, k0, v0, k1, v1, m = R.case(*c)
    sp = lambda t: t.double().reshape(B, -1, heads, 64)      # noqa: E731
    q, k0, v0, k1, v1 = sp(q), sp(k0), sp(v0), sp(k1), sp(v1)
    out = torch.zeros(B, Nq, heads, 64, dtype=torch.float64)
    for b in range(B):
        for h in range(heads):
            out[b, :, h] = w0 * torch.softmax(q[b, :, h] @ k0[b, :, h].T / 8.0, -1) @ v0[b, :, h] + fn(q[b, :, h], k1[b, :, h], v1[b, :, h], m[b].double(), float(torch.tensor(R.S_B[b], dtype=torch.float32)))
    return out.reshape(B, Nq, heads * 64)


def test_faults_leave_the_bound():
    c = ("diffuse",) + R.MASK_SWEEP[1]      # soft ramps, G = 3
    G = c[5]
    right = lambda q, k, v, m, s: sum(s * m[g].reshape(-1, 1) * (torch.softmax(q @ k[4 * g:4 * g + 4].T / 8.0, -1) @ v[4 * g:4 * g + 4]) for g in range(G))      # noqa: E731
    assert _worst(c, _groups(c, right)) < 1e-6
    one_softmax = lambda q, k, v, m, s: (torch.softmax(q @ k.T / 8.0, -1) * s * m.T.repeat_interleave(4, 1)) @ v      # noqa: E731  one softmax over all groups' keys
    shifted = lambda q, k, v, m, s: sum(s * m[(g + 1) % G].reshape(-1, 1) * (torch.softmax(q @ k[4 * g:4 * g + 4].T / 8.0, -1) @ v[4 * g:4 * g + 4]) for g in range(G))      # noqa: E731
    row0 = lambda q, k, v, m, s: sum(R.S_B[0] * m[g].reshape(-1, 1) * (torch.softmax(q @ k[4 * g:4 * g + 4].T / 8.0, -1) @ v[4 * g:4 * g + 4]) for g in range(G))      # noqa: E731
    offby = lambda q, k, v, m, s: sum(s * m[g].reshape(-1, 1) * (torch.softmax(q @ k[4 * g + 1:4 * g + 5].T / 8.0, -1) @ v[4 * g + 1:4 * g + 5]) for g in range(G))      # noqa: E731
    for name, fn in (("one softmax over every group", one_softmax), ("group g weighted by the mask of g + 1", shifted), ("s[0] for every row", row0), ("groups one key off", offby)):
        r = _worst(c, _groups(c, fn))
        print(f"[region-attn] fault `{name}`: max(err / bound) {r:.3g}")
        assert r > 1.0


# ---- the pyramid ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["binary", "soft"])
def test_levels_reference_is_avg_pool(kind):
    for h, w in R.LEVEL_HW:
        m = R.levels_case(kind, h, w)
        for f in R.LEVEL_F + (8,) if h % 8 == 0 and w % 8 == 0 else R.LEVEL_F:
            want = F.avg_pool2d(m.double().reshape(-1, 1, h, w), f).reshape(R.LEVEL_B, R.LEVEL_G, -1)
            got = R.levels(m, f)
            assert torch.equal(got, R.round16(want))
            if kind == "binary":
                assert torch.equal(got, want)      # {0, 1} masks: exact in fp16
            # the kernel's arithmetic, restated: an fp32 sum in row-major order, the exact 1 / f^2, one rounding
            acc = torch.zeros(R.LEVEL_B, R.LEVEL_G, h // f, w // f, dtype=torch.float32)
            for dy in range(f):
                for dx in range(f):
                    acc = acc + m[:, :, dy::f, dx::f].float()
            assert torch.equal((acc * (1.0 / (f * f))).half().double().reshape(R.LEVEL_B, R.LEVEL_G, -1), got)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch(lib):
    """every call below is refused on the host: the pointers are never dereferenced and no GPU is needed"""
    INVALID, SHAPE = 1, 2
    p, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    L = lib

    def att(Q=p, ldq=64, O=p, ldo=64, nseg=2, K0=p, V0=p, ld0=128, n0=77, w0=1.0, K1=p, V1=p, ld1=128, n1=12, rw=p, G=3, B=1, heads=1, Nq=128):
        return L.ia2p_attention_regions(None, Q, ldq, O, ldo, B, heads, Nq, nseg, K0, V0, ld0, n0, w0, K1, V1, ld1, n1, 1.0, rw, G, None)

    lev = lambda m=p, o=p, B=1, G=3, h=16, w=16, f=2: L.ia2p_region_levels(None, m, o, B, G, h, w, f)      # noqa: E731
    cases = [
        (att(Q=None), INVALID), (att(O=None), INVALID), (att(K0=None), INVALID), (att(V0=None), INVALID), (att(K1=None), INVALID), (att(V1=None), INVALID),
        (att(rw=None), INVALID), (att(w0=0.0), INVALID), (att(w0=-0.0), INVALID), (att(nseg=1), INVALID), (att(nseg=3), INVALID),
        (att(G=0, n1=0), SHAPE), (att(G=-1, n1=-4), SHAPE), (att(G=17, n1=68), SHAPE), (att(G=3, n1=8), SHAPE), (att(G=3, n1=16), SHAPE), (att(G=3, n1=13), SHAPE),
        (att(ldq=68), SHAPE), (att(ldo=68), SHAPE), (att(ld0=132), SHAPE), (att(ld1=132), SHAPE), (att(O=odd), SHAPE), (att(n0=0), SHAPE), (att(Nq=0), SHAPE),
        (att(B=0), SHAPE), (att(heads=0), SHAPE),
        (lev(m=None), INVALID), (lev(o=None), INVALID), (lev(f=0), INVALID), (lev(f=3), INVALID), (lev(f=16), INVALID), (lev(f=-2), INVALID),
        (lev(h=18, f=4), SHAPE), (lev(w=18, f=4), SHAPE), (lev(h=4, f=8), SHAPE), (lev(B=0), SHAPE), (lev(G=0), SHAPE), (lev(h=0), SHAPE),
    ]
    for i, (got, want) in enumerate(cases):
        assert got == want, f"case {i}: status {got}, expected {want}"
    assert L.ia2p_last_error(None)


# ---- the padding rule and the union mask (inpaint.py / batch.py), on CPU tensors ----------------------------------------------------------------------------
def test_padding_rule_and_union_mask():
    from instructany2pix_amd.batch import pad_subjects
    from instructany2pix_amd.inpaint import prepare_mask, prepare_region_masks, union_mask
    h = w = 16
    mk = lambda y0, y1, x0, x1: torch.zeros(128, 128).index_put_((torch.arange(y0, y1)[:, None], torch.arange(x0, x1)[None, :]), torch.tensor(1.0))      # noqa: E731
    a, b, c = mk(0, 64, 0, 64), mk(32, 96, 32, 96), mk(100, 128, 0, 16)
    ea, eb, ec = (torch.full((64,), float(i + 1)) for i in range(3))
    regions, embeds, G = pad_subjects([([a], [ea]), ([a, b, c], [ea, eb, ec])], h, w, "cpu")
    assert G == 3 and regions.shape == (2, 3, h, w) and embeds.shape == (6, 64) and regions.dtype == embeds.dtype == torch.float16
    assert torch.equal(regions[0, 0], prepare_mask(a, h, w, "cpu")[0, 0]) and torch.equal(regions[1, 2], prepare_mask(c, h, w, "cpu")[0, 0])
    assert bool((regions[0, 1:] == 0).all()) and bool((embeds[1:3] == 0).all())      # the padding: all-zero masks, zero embeddings
    assert torch.equal(embeds[0], ea.half()) and torch.equal(embeds[3:], torch.stack([ea, eb, ec]).half())
    u = union_mask(regions)
    assert u.shape == (2, 1, h, w) and torch.equal(u[0, 0], regions[0, 0]) and torch.equal(u[1, 0], torch.maximum(torch.maximum(regions[1, 0], regions[1, 1]), regions[1, 2]))
    assert set(u.unique().tolist()) == {0.0, 1.0}
    # the forms `region_masks=` takes agree
    lst, t3, t4 = prepare_region_masks([a, b, c], h, w, "cpu"), prepare_region_masks(torch.stack([a, b, c]), h, w, "cpu"), prepare_region_masks(torch.stack([a, b, c])[None], h, w, "cpu")
    assert lst.shape == (1, 3, h, w) and torch.equal(lst, t3) and torch.equal(lst, t4) and torch.equal(lst[0], regions[1])
    with pytest.raises(ValueError):
        pad_subjects([([a, b], [ea])], h, w, "cpu")
    with pytest.raises(ValueError):
        pad_subjects([([a] * 17, [ea] * 17)], h, w, "cpu")
    with pytest.raises(ValueError):
        prepare_region_masks([], h, w, "cpu")


def test_joint_arguments_are_refused_on_the_host():
    from types import SimpleNamespace
    from instructany2pix_amd.batch import edit_batch
    with pytest.raises(ValueError, match="subject_modes"):
        edit_batch(SimpleNamespace(ip_adapter_xl=None, vae=None), ["a"], [[]], subject_modes="both")
