"""Host side of the ImageBind front end (instructany2pix_amd/imagebind.py): the audio and image transforms against independent restatements, the ViT
executor's plan / validation (host-only, as `ia2p_clip_create` is), the checkpoint key table, and the pipeline's mm_data resolution order. No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from instructany2pix_amd import imagebind as ib


@pytest.fixture(scope="module")
def lib():
    from instructany2pix_amd import build, _ffi
    build.build(verbose=False)
    return _ffi.lib()


def _signal(seconds, sr=16000, seed=3):
    g = np.random.default_rng(seed)
    t = np.arange(int(seconds * sr)) / sr
    return (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * np.sin(2 * np.pi * 3100 * t + 1.0) + 0.05 * g.standard_normal(t.size)).astype(np.float32)


def test_fbank_matches_the_numpy_kaldi_path_of_transformers():
    """the same Kaldi fbank through `transformers.audio_utils` (what ASTFeatureExtractor runs without torchaudio), driven with ImageBind's settings"""
    from transformers.audio_utils import mel_filter_bank, spectrogram, window_function
    x = _signal(2.0)
    x = x - x.mean()
    got = ib.kaldi_fbank(x).T
    assert got.shape == (128, 198) and got.dtype == np.float32
    # (257 = 512 / 2 + 1 frequency bins, as ASTFeatureExtractor passes: the function derives the bin width from that count)
    filters = mel_filter_bank(num_frequency_bins=257, num_mel_filters=128, min_frequency=20, max_frequency=8000, sampling_rate=16000, norm=None,
                              mel_scale="kaldi", triangularize_in_mel_space=True)
    ref = spectrogram(x, window_function(400, "hann", periodic=False), frame_length=400, hop_length=160, fft_length=512, power=2.0, center=False,
                      preemphasis=0.97, mel_filters=filters, log_mel="log", mel_floor=1.192092955078125e-07, remove_dc_offset=True)
    assert ref.shape == (128, 198)
    diff = float(np.abs(got - ref).max())
    print("fbank max abs difference (log units):", diff)
    assert diff <= 1e-3


def test_clip_times_and_padding():
    assert ib.clip_timepoints(10.0) == [(0.0, 2.0), (4.0, 6.0), (8.0, 10.0)]
    assert ib.clip_timepoints(2.0) == [(0.0, 2.0)] * 3
    assert ib.clip_timepoints(1.0) == [(0.0, 2.0)] * 3
    ten = ib.waveform_to_clips(_signal(10.0)[None], 16000)
    assert ten.shape == (3, 1, 128, 204) and ten.dtype == np.float32
    pad = (0.0 + 4.268) / 9.138                                     # zero-padding happens before (x - mean) / std
    assert np.allclose(ten[:, :, :, 198:], pad) and not np.allclose(ten[:, :, :, 197], pad)
    assert not np.array_equal(ten[0], ten[1]) and not np.array_equal(ten[1], ten[2])
    x = _signal(10.0)                                               # clip 1 is seconds 4 .. 6, its own mean removed
    c = x[64000:96000]
    assert np.allclose(ten[1, 0, :, :198], (ib.kaldi_fbank(c - c.mean()).T + 4.268) / 9.138, atol=1e-5)
    one = ib.waveform_to_clips(_signal(1.0)[None], 16000)           # shorter than a clip: the whole file three times, 98 frames
    assert one.shape == (3, 1, 128, 204) and np.array_equal(one[0], one[1]) and np.array_equal(one[0], one[2])
    assert np.allclose(one[:, :, :, 98:], pad) and not np.allclose(one[:, :, :, 97], pad)
    long_ = ib.waveform_to_clips(_signal(3.0)[None], 16000, target_length=100)      # longer than the target: cropped
    assert long_.shape == (3, 1, 128, 100)
    half = ib.waveform_to_clips(_signal(4.0, sr=8000)[None], 8000)                 # another sample rate is resampled to 16 kHz
    assert half.shape == (3, 1, 128, 204) and np.isfinite(half).all()


def test_wav_int16_and_float32_load_alike(tmp_path):
    from scipy.io import wavfile
    # the same samples in both encodings: on the int16 grid, so that the comparison checks the decoding convention (int16 / 32768) and not the 16-bit
    # quantisation noise (which moves log energies near spectral nulls by more than 1e-3 on its own)
    q = np.round(_signal(3.0) * 32768.0).clip(-32768, 32767).astype(np.int16)
    x = q.astype(np.float32) / 32768.0
    wavfile.write(tmp_path / "f.wav", 16000, x)
    wavfile.write(tmp_path / "i.wav", 16000, q)
    stereo = np.stack([x, -x], axis=1)
    wavfile.write(tmp_path / "s.wav", 16000, stereo)
    f = ib.load_and_transform_audio_data([str(tmp_path / "f.wav")], "cpu")
    i = ib.load_and_transform_audio_data([str(tmp_path / "i.wav")], "cpu")
    assert f.shape == i.shape == (1, 3, 1, 128, 204) and f.dtype == torch.float32
    d = float((f - i).abs().max())
    print("int16 vs float32 WAV, max abs difference:", d)
    assert d <= 1e-3
    w, sr = ib.read_wav(str(tmp_path / "s.wav"))
    assert w.shape == (2, 48000) and sr == 16000 and np.array_equal(w[0], x)
    both = ib.load_and_transform_audio_data([str(tmp_path / "f.wav"), str(tmp_path / "i.wav")], "cpu")
    assert both.shape == (2, 3, 1, 128, 204) and torch.equal(both[0], f[0])


@pytest.mark.parametrize("w,h", [(300, 200), (200, 300)])
def test_image_transform(w, h, tmp_path):
    from PIL import Image
    g = np.random.default_rng(w)
    a = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img = Image.fromarray(a)
    got = ib.transform_image(img)
    assert got.shape == (3, 224, 224) and got.dtype == torch.float32
    # numpy restatement: shorter side -> 224 (long side int(224 * long / short) = 336), centre crop at round((336 - 224) / 2) = 56
    nw, nh = (336, 224) if w > h else (224, 336)
    r = np.asarray(img.resize((nw, nh), Image.BICUBIC), dtype=np.float32) / 255.0
    top, left = (0, 56) if w > h else (56, 0)
    r = r[top:top + 224, left:left + 224]
    r = (r - np.array([0.48145466, 0.4578275, 0.40821073], np.float32)) / np.array([0.26862954, 0.26130258, 0.27577711], np.float32)
    assert np.allclose(got.numpy(), r.transpose(2, 0, 1), atol=1e-6)
    img.save(tmp_path / "x.png")
    batch = ib.load_and_transform_vision_data([str(tmp_path / "x.png"), img], "cpu")
    assert batch.shape == (2, 3, 224, 224) and torch.equal(batch[0], got) and torch.equal(batch[1], got)
    grey = ib.transform_image(img.convert("L"))                     # converted to RGB: three equal planes before normalisation
    assert grey.shape == (3, 224, 224)


def _create(lib, t):
    from instructany2pix_amd import _ffi
    h = C.c_void_p()
    _ffi.check(lib.ia2p_vit_create(C.byref(_ffi.make_vit_config(t)), C.byref(h)), None, vit=True)
    return h


def test_vit_create_plans_both_towers_and_refuses_bad_shapes(lib):
    from dataclasses import replace
    from instructany2pix_amd.weights import param_count
    cfg = ib.imagebind_huge_config()
    for m, tokens in (("vision", 257), ("audio", 229)):
        t = getattr(cfg, m)
        h = _create(lib, t)
        assert lib.ia2p_vit_tokens(h) == tokens == t.tokens
        n = param_count(ib.imagebind_param_specs(cfg, (m,)))
        if m == "vision":
            n -= t.hidden_size * 3 * 14 * 14                        # the Conv3d stem is held summed over its two time steps
        arena = lib.ia2p_vit_arena_bytes(h)
        assert 2 * n <= arena < 2 * n * 1.6 + (1 << 20)             # + the gamma-folded copies of the QKV and fc1 weights (7 of 12 H^2 per block)
        assert 0 < lib.ia2p_vit_workspace_bytes(h, 1) < lib.ia2p_vit_workspace_bytes(h, 3)      # sizing is a host dry run
        assert lib.ia2p_vit_workspace_bytes(h, 0) == 0
        lib.ia2p_vit_destroy(h)
    v = cfg.vision
    for bad in (replace(v, hidden_size=1248, num_heads=16),          # hidden not a multiple of 64
                replace(v, hidden_size=1536, num_heads=16),          # head dim 96
                replace(v, hidden_size=128, num_heads=4),            # head dim 32
                replace(v, image_h=8),                               # a 14 x 14 patch does not fit
                replace(v, image_h=448, image_w=448)):               # 1025 tokens: more keys than the attention launch holds
        with pytest.raises(ValueError):
            _create(lib, bad)
    assert lib.ia2p_vit_last_error(None)


class _StubTower:
    def __init__(self):
        self.loaded, self.final = {}, False

    def load_tensor(self, k, v):
        self.loaded[k] = tuple(v.shape)

    def finalize(self):
        self.final = True


def _six_modality_keys(cfg):
    keys = {k: shp for k, shp, _ in ib.imagebind_param_specs(cfg)}
    keys["modality_postprocessors.audio.1.log_logit_scale"] = ()
    for m in ("text", "depth", "thermal", "imu"):
        keys[f"modality_preprocessors.{m}.pos_embedding_helper.pos_embed"] = (1, 8, 16)
        keys[f"modality_trunks.{m}.blocks.0.attn.in_proj_weight"] = (48, 16)
        keys[f"modality_heads.{m}.proj.1.weight"] = (1024, 16)
        keys[f"modality_postprocessors.{m}.1.log_logit_scale"] = ()
    keys["modality_preprocessors.text.token_embedding.weight"] = (100, 16)
    keys["modality_preprocessors.imu.rgbt_stem.proj.weight"] = (16, 48)
    return keys


def test_key_table():
    cfg = ib.imagebind_tiny_config()
    model = object.__new__(ib.HipImageBindModel)
    model.config, model.modalities, model.towers = cfg, ("vision", "audio"), {"vision": _StubTower(), "audio": _StubTower()}
    sd = {k: torch.zeros(shp) for k, shp in _six_modality_keys(cfg).items()}
    model.load_state_dict(sd, strict=True)
    v, a = model.towers["vision"], model.towers["audio"]
    assert v.final and a.final
    assert v.loaded["stem.weight"] == (320, 3, 2, 14, 14) and a.loaded["stem.weight"] == (128, 1, 16, 16)
    assert v.loaded["pos_embed"] == (1, 257, 320) and a.loaded["pos_embed"] == (1, 229, 128)
    assert "pre_ln.weight" in v.loaded and "pre_ln.weight" not in a.loaded and "stem.norm.bias" in a.loaded and "stem.norm.bias" not in v.loaded
    assert "blocks.1.attn.bias_k" in a.loaded and "blocks.1.attn.bias_k" not in v.loaded
    assert {"cls_token", "head.norm.weight", "head.norm.bias", "head.proj.weight", "blocks.0.mlp.fc2.bias", "blocks.1.norm_2.weight"} <= set(v.loaded)
    assert len(v.loaded) == 8 + 2 * 12 and len(a.loaded) == 8 + 2 * 14
    bad = dict(sd)
    bad["modality_trunks.vision.pre_transformer_layer.O.weight"] = bad.pop("modality_trunks.vision.pre_transformer_layer.0.weight")
    with pytest.raises(KeyError):
        model.load_state_dict(bad, strict=True)
    with pytest.raises(KeyError):
        model.load_state_dict({"visual.proj": torch.zeros(1)}, strict=True)
    model.load_state_dict(bad, strict=False)                       # tolerated without strict


def test_key_table_against_the_executor(lib):
    """every tower key the table produces is one the executor registers. Host-only: an arena ADDRESS is bound (never dereferenced) and each tensor is offered
    with one element, which the executor refuses with IA2P_ERR_SHAPE for a key it knows and IA2P_ERR_KEY for one it does not, before any copy."""
    cfg = ib.imagebind_tiny_config()
    for m in ("vision", "audio"):
        h = _create(lib, getattr(cfg, m))
        assert lib.ia2p_vit_bind_arena(h, C.c_void_p(1 << 20), lib.ia2p_vit_arena_bytes(h)) == 0
        shape = (C.c_int64 * 1)(1)
        seen = set()
        for k, _, _ in ib.imagebind_param_specs(cfg, (m,)):
            mod, tk = ib.tower_key(k, cfg)
            assert mod == m and tk and tk not in seen
            seen.add(tk)
            assert lib.ia2p_vit_load_tensor(h, tk.encode(), C.c_void_p(1 << 20), shape, 1, None) == 2, (k, tk)
        assert lib.ia2p_vit_load_tensor(h, b"blocks.0.attn.nope", C.c_void_p(1 << 20), shape, 1, None) == 3
        with pytest.raises(KeyError):                                # nothing was loaded: finalize names a missing parameter
            from instructany2pix_amd import _ffi
            _ffi.check(lib.ia2p_vit_finalize_weights(h), h, vit=True)
        lib.ia2p_vit_destroy(h)


class _StubImageBind:
    device = "cpu"

    def __init__(self):
        self.calls = []

    def __call__(self, inputs):
        (m, x), = inputs.items()
        self.calls.append((m, tuple(x.shape)))
        g = torch.Generator().manual_seed(len(m))
        return {m: torch.randn(x.shape[0], 1024, generator=g) * (3.0 if m == "audio" else 1.0)}


def test_modality_embeds_resolution_order(tmp_path):
    from PIL import Image
    from scipy.io import wavfile
    from instructany2pix_amd.pipeline import InstructAny2PixPipeline
    Image.fromarray(np.full((40, 60, 3), 90, np.uint8)).save(tmp_path / "a.png")
    wavfile.write(tmp_path / "c.wav", 16000, _signal(2.5))
    img, wav = {"type": "image", "fname": str(tmp_path / "a.png")}, {"type": "audio", "fname": str(tmp_path / "c.wav")}
    p = InstructAny2PixPipeline(unet=object())
    assert p.model_imb is None and p.modality_encoder is None
    with pytest.raises(ValueError, match="entry\\['embed'\\] or the pipeline built with modality_encoder="):
        p._modality_embeds([img])
    given = torch.arange(1024.0)
    out = p._modality_embeds([{"embed": given}])                    # as before: a ready-made vector needs nothing else
    assert out.shape == (1, 1024) and torch.allclose(out[0], given / given.norm() * 20)
    stub = _StubImageBind()
    p = InstructAny2PixPipeline(unet=object(), imagebind=stub)
    assert p.model_imb is stub
    pil = Image.open(tmp_path / "a.png")
    out = p._modality_embeds([img, wav, {"type": "image", "fname": pil}, {"type": "image", "embed": given}])
    assert out.shape == (4, 1024) and out.dtype == torch.float32
    assert torch.allclose(out.norm(dim=-1), torch.full((4,), 20.0), atol=1e-4)
    assert stub.calls == [("vision", (2, 3, 224, 224)), ("audio", (1, 3, 1, 128, 204))]      # the two images as one batch; the embed entry never reaches the model
    assert torch.allclose(out[3], given / given.norm() * 20)
    p.modality_encoder = lambda r: torch.ones(1024)                 # a user's encoder takes precedence over the model
    stub.calls.clear()
    out = p._modality_embeds([img, {"embed": given}])
    assert stub.calls == [] and torch.allclose(out[0], torch.full((1024,), 20.0 / 32.0)) and torch.allclose(out[1], given / given.norm() * 20)
    p.modality_encoder = None
    with pytest.raises(ValueError):
        p._modality_embeds([{"type": "video", "fname": "x.mp4"}])
    with pytest.raises(ValueError):
        p._modality_embeds([])
