"""The device sampler without a GPU: the Philox restatement the GPU tests judge the kernel's uniform by, the two new symbols of the library, and the
argument checks of the `sampler` / `seeds` keywords (made before anything touches a device)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sampler_ref  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def test_philox_restatement_reproduces_the_known_answers():
    """Random123's known-answer vectors for philox4x32 with ten rounds (kat_vectors): counter and key all zero, and all ones"""
    assert sampler_ref.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert sampler_ref.philox4x32_10((ones,) * 4, (ones,) * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_uniform_is_24_bits_of_word_0_under_the_split_seed():
    seed, step = (0x89ABCDEF << 32) | 0x01234567, 77
    w0 = sampler_ref.philox4x32_10((step, 0, 0, 0), (0x01234567, 0x89ABCDEF))[0]
    u = sampler_ref.uniform(seed, step)
    assert u.dtype == np.float32 and float(u) == (w0 >> 8) / 2.0 ** 24 and 0.0 <= float(u) < 1.0
    us = [float(sampler_ref.uniform(3, s)) for s in range(64)]
    assert len(set(us)) == 64 and sampler_ref.uniform(3, 5) != sampler_ref.uniform(4, 5)


def test_oracle_is_sample_probs():
    from instructany2pix_amd.llm import sample_probs
    row = torch.randn(1000, generator=torch.Generator().manual_seed(2)) * 3
    for top_k, n in ((50, 50), (0, 1000), (1007, 1000)):
        kept, probs, cdf = sampler_ref.oracle(row, 0.3, top_k)
        assert int(kept.sum()) == n == cdf.numel() and abs(float(cdf[-1]) - 1) < 1e-12
        assert torch.allclose(probs.float(), sample_probs(row[None], 0.3, top_k if top_k else None)[0], rtol=1e-5, atol=1e-12)


def test_library_exports_the_sampler_and_the_device_token_decode(lib):
    assert hasattr(lib, "ia2p_sample_tokens") and hasattr(lib, "ia2p_llm_decode_batch_dev")
    one = 256           # never dereferenced: every call below is refused before any HIP call
    import ctypes as C
    s1, t1 = (C.c_uint64 * 1)(1), (C.c_uint32 * 1)(0)
    assert lib.ia2p_sample_tokens(None, None, 8, 1, 8, 1.0, 0, 1, s1, t1, one, None, None) == 1
    assert lib.ia2p_sample_tokens(None, one, 8, 1, 8, 1.0, 0, 1, None, t1, one, None, None) == 1          # sampling without seeds
    assert lib.ia2p_sample_tokens(None, one, 8, 1, 8, 0.0, 0, 1, s1, t1, one, None, None) == 1            # temperature 0
    assert lib.ia2p_sample_tokens(None, one, 8, 1, 8, 1.0, 0, 2, s1, t1, one, None, None) == 1
    assert lib.ia2p_sample_tokens(None, one, 8, 0, 8, 1.0, 0, 1, s1, t1, one, None, None) == 2
    assert lib.ia2p_sample_tokens(None, one, 8, 4097, 8, 1.0, 0, 0, None, None, one, None, None) == 2
    assert lib.ia2p_sample_tokens(None, one, 8, 1, (1 << 20) + 1, 1.0, 0, 1, s1, t1, one, None, None) == 2
    assert lib.ia2p_sample_tokens(None, one, 7, 2, 8, 1.0, 0, 1, s1, t1, one, None, None) == 2            # rows that overlap
    assert b"sample_tokens" in lib.ia2p_last_error(None)
    assert lib.ia2p_llm_decode_batch_dev(None, None, None, None, None, 1, one, one, one, 1 << 20) == 1


def test_sampler_and_seeds_arguments_are_checked_before_any_device_work():
    from instructany2pix_amd.config import tiny_llm
    from instructany2pix_amd.llm import HipInstructAny2PixLM
    with pytest.raises(ValueError, match="sampler"):
        HipInstructAny2PixLM(tiny_llm(), sampler="nonsense")
    lm = object.__new__(HipInstructAny2PixLM)          # no engine behind it: the checks below come before the first use of one
    lm.sampler = "host"
    prompts = [torch.tensor([[1, 5, 6]]), torch.tensor([[1, 7]])]
    for sampler in ("host", "device", None):
        with pytest.raises(ValueError, match="seeds"):
            lm.generate_batch(prompts, sampler=sampler, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="sampler"):
        lm.generate_batch(prompts, sampler="nonsense")
    with pytest.raises(ValueError, match="sampler"):
        lm.generate(prompts[0], sampler="gpu")
