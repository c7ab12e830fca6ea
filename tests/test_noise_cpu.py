"""The noise rule of include/ia2p.h ("Seeded noise") on the CPU: the float64 restatement of tests/noise_ref.py reproduces Philox's known answers, the three entry
points are declared and exported, and the restatement itself is a standard normal to six standard errors of its first four moments. Needs no GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref  # noqa: E402
import sampler_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 0xFFFFFFFF
SEEDS = (0, 1, 0x0123456789ABCDEF, 2 ** 63 - 1)
DRAWS = (0, 1, 3)


def test_block_function_reproduces_the_known_answers_and_the_scalar_restatement():
    """Random123's known-answer vectors (kat_vectors, philox4x32 with ten rounds), and the vectorised twin against tests/sampler_ref.py word for word"""
    zero = noise_ref.philox_blocks(np.array([0], dtype=np.uint64), 0, 0, 0, (0, 0))[:, 0]
    ones = noise_ref.philox_blocks(np.array([ONES], dtype=np.uint64), ONES, ONES, ONES, (ONES, ONES))[:, 0]
    assert [int(w) for w in zero] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(w) for w in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    seed, draw = 0x0123456789ABCDEF, 3
    key = (seed & ONES, seed >> 32)
    js = np.array([0, 1, 7, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    got = noise_ref.philox_blocks(js, draw, 0, 1, key)
    for col, j in enumerate(js):
        assert [int(w) for w in got[:, col]] == sampler_ref.philox4x32_10((int(j), draw, 0, 1), key), int(j)


def test_rule_maps_words_to_elements_as_the_header_says():
    """element e: block e >> 2, pair (e & 3) >> 1, cosine for even e and sine for odd e; a sub-range is the same elements"""
    seed, draw = 0x0123456789ABCDEF, 1
    z, r = noise_ref.normals(seed, draw, 23)
    for e in (0, 1, 2, 3, 4, 13, 22):
        w = sampler_ref.philox4x32_10((e >> 2, draw, 0, 1), (seed & ONES, seed >> 32))
        p = (e & 3) >> 1
        u1, u2 = ((w[2 * p] >> 8) + 1) * 2.0 ** -24, (w[2 * p + 1] >> 8) * 2.0 ** -24
        rr = np.sqrt(-2 * np.log(u1))
        want = rr * (np.sin(2 * np.pi * u2) if e & 1 else np.cos(2 * np.pi * u2))
        assert abs(z[e] - want) < 1e-12 and abs(r[e] - rr) < 1e-15, e
    z2, _ = noise_ref.normals(seed, draw, 9, first=12)
    assert np.array_equal(z2, z[12:21])
    assert not np.array_equal(noise_ref.normals(seed, draw + 1, 23)[0], z)
    # the domain tag: block 0 of draw 0 is not the sampler's block at step 0 for the same seed
    assert noise_ref.philox_blocks(np.array([0], dtype=np.uint64), 0, 0, 1, (seed & ONES, seed >> 32))[0, 0] != \
        sampler_ref.philox4x32_10((0, 0, 0, 0), (seed & ONES, seed >> 32))[0]


def test_entry_points_are_declared_bound_and_exported():
    from instructany2pix_amd import _ffi, build
    hdr = open(os.path.join(ROOT, "include", "ia2p.h")).read()
    build.build(verbose=False)
    lib = _ffi.lib()
    for name in ("ia2p_randn_seeded", "ia2p_posterior_sample_seeded", "ia2p_polar_mix_v"):
        assert re.search(r"\bia2p_status\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ia2p.h"
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    assert "noise.hip" in build.SOURCES
    from instructany2pix_amd import noise
    assert (noise.DRAW_BASE_POSTERIOR, noise.DRAW_POLAR, noise.DRAW_HANDOFF_POSTERIOR, noise.DRAW_REFINER, noise.DRAW_INPAINT) == (0, 1, 2, 3, 4)
    assert noise.inpaint_draw(2) == 6


def test_refusals_need_no_device():
    """every refusal is decided on the host before a launch: the codes come back on a machine without a GPU (the pointers are never dereferenced)"""
    import ctypes as C
    from instructany2pix_amd import _ffi, build
    build.build(verbose=False)
    L = _ffi.lib()
    seeds, draws, alphas = (C.c_uint64 * 2)(1, 2), (C.c_uint32 * 2)(0, 0), (C.c_float * 2)(0.5, 0.5)
    p = C.c_void_p(4096)            # a non-null, 16-byte aligned address that is never touched
    assert L.ia2p_randn_seeded(None, None, 0, 2, 16, 0, seeds, draws) == 1
    assert L.ia2p_randn_seeded(None, p, 0, 2, 16, 0, None, draws) == 1
    assert L.ia2p_randn_seeded(None, p, 2, 2, 16, 0, seeds, draws) == 1
    assert L.ia2p_randn_seeded(None, p, 0, 0, 16, 0, seeds, draws) == 2
    assert L.ia2p_randn_seeded(None, p, 0, 2, 0, 0, seeds, draws) == 2
    assert L.ia2p_randn_seeded(None, p, 0, 2, 16, 6, seeds, draws) == 2
    assert L.ia2p_randn_seeded(None, p, 0, 2, 16, -4, seeds, draws) == 2
    assert L.ia2p_randn_seeded(None, p, 0, 2, 2 ** 34 - 4, 8, seeds, draws) == 2
    assert b"2^34" in L.ia2p_last_error(None)
    assert L.ia2p_posterior_sample_seeded(None, None, p, 2, 4, 16, 1.0, seeds, draws) == 1
    assert L.ia2p_posterior_sample_seeded(None, p, p, 2, 0, 16, 1.0, seeds, draws) == 2
    assert L.ia2p_posterior_sample_seeded(None, p, p, 0, 4, 16, 1.0, seeds, draws) == 2
    assert L.ia2p_polar_mix_v(None, p, p, None, p, 2, 16) == 1
    assert L.ia2p_polar_mix_v(None, p, p, alphas, p, 2, 0) == 2
    assert L.ia2p_polar_mix_v(None, p, p, alphas, p, 0, 16) == 2
    with pytest.raises(ValueError, match="SHAPE"):
        _ffi.check(L.ia2p_polar_mix_v(None, p, p, alphas, p, 0, 16))


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_is_a_standard_normal(seed, draw):
    """n = 2^20 values per (seed, draw): every estimate within six standard errors of its N(0, 1) value, and no value past the rule's ceiling"""
    n = 1 << 20
    z, _ = noise_ref.normals(seed, draw, n)
    mean, var, skew, kurt, top = noise_ref.moments4(z)
    cm, cv, cs, ck, ctop = noise_ref.moment_caps(n)
    print(f"seed {seed:#x} draw {draw}: mean {mean:.2e} var-1 {var - 1:.2e} skew {skew:.2e} kurt {kurt:.2e} max {top:.3f}")
    assert abs(mean) < cm and abs(var - 1) < cv and abs(skew) < cs and abs(kurt) < ck and top <= ctop


def test_seed_helpers():
    import torch
    from instructany2pix_amd import noise
    assert noise.resolve_seeds(None, 3) == [None] * 3
    assert noise.resolve_seeds(5, 3) == [5, 6, 7] and noise.resolve_seeds(2 ** 64 - 1, 2) == [2 ** 64 - 1, 0]
    assert noise.resolve_seeds([9, None, 2 ** 64 - 1], 3) == [9, None, 2 ** 64 - 1]
    for bad in ([1, 2], [-1, 0, 0], [2 ** 64, 0, 0]):
        with pytest.raises(ValueError):
            noise.resolve_seeds(bad, 3)
    torch.manual_seed(3)
    a = noise.seeds_from_global(4)
    torch.manual_seed(3)
    from instructany2pix_amd.llm import _resolve_seeds
    assert a == _resolve_seeds(None, 4) and all(0 <= s < 2 ** 63 for s in a) and len(set(a)) == 4


def test_request_seed_reaches_the_llm_only_under_its_device_sampler():
    """the request's seed keys its token stream where the LLM samples on the device (`generate(seed=)`, `generate_batch(seeds=)`); the host sampler keeps the
    global generator and is handed nothing (stand-in LLM: the wiring needs no GPU)"""
    from types import SimpleNamespace
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    pipe = object.__new__(InstructAny2PixPipeline)
    seen = []
    lm = SimpleNamespace(sampler="device", DEFAULT_VIDEO_TOKEN_IDX=1, eval=lambda: None,
                         generate=lambda ids, **kw: seen.append(("one", kw.get("seed", "absent"))),
                         generate_batch=lambda prompts, **kw: seen.append(("batch", kw.get("seeds", "absent"))))
    pipe.any2pix_lm = lm
    pipe._llm_request = lambda inst, aux: ("ids", {}, None)
    reqs = [("ids", {}, None)] * 2
    pipe._llm_generate("inst", None, seed=7)
    pipe._llm_generate("inst", None)
    pipe._llm_generate_batch(reqs, seeds=[7, 8])
    pipe._llm_generate_batch(reqs)
    lm.sampler = "host"
    pipe._llm_generate("inst", None, seed=7)
    pipe._llm_generate_batch(reqs, seeds=[7, 8])
    assert seen == [("one", 7), ("one", "absent"), ("batch", [7, 8]), ("batch", "absent"), ("one", "absent"), ("batch", "absent")]
