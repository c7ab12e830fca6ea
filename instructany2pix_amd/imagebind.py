"""ImageBind's image and audio encoders on the HIP kernels: mm_data files -> 1024-d embeddings (reference pipeline.py:118-121, :155-168).

  HipImageBindModel(config)                  <- `imagebind_model.imagebind_huge(pretrained=True)`; `model({'vision': x})['vision']`, `model({'audio': x})['audio']`
  ModalityType                               <- `imagebind.models.imagebind_model.ModalityType`
  load_and_transform_vision_data(paths, dev) <- `imagebind.data.load_and_transform_vision_data` (PIL bicubic resize 224, centre crop, CLIP mean / std)
  load_and_transform_audio_data(paths, dev)  <- `imagebind.data.load_and_transform_audio_data` (3 clips of 2 s, Kaldi fbank 128 x 204, mean / std)

Each tower runs through `ia2p_vit_encode` (csrc/vit_engine.hip); the transforms run on the host in numpy (612 frames per file). The `imagebind` package and
its checkpoint were not at hand where this was written: the architecture is restated from knowledge of `imagebind_huge` and parity with the real package is
unpinned. WAV files only (scipy.io.wavfile); other sample rates go through scipy's polyphase resampler, which is NOT torchaudio's
(windowed-sinc) resampler and differs from it in the last digits.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _ffi

ModalityType = SimpleNamespace(VISION="vision", TEXT="text", AUDIO="audio", THERMAL="thermal", DEPTH="depth", IMU="imu")
_SKIPPED = (ModalityType.TEXT, ModalityType.THERMAL, ModalityType.DEPTH, ModalityType.IMU)


@dataclass
class ViTTowerConfig:
    """one tower, field for field `ia2p_vit_config` (include/ia2p.h)"""
    hidden_size: int
    num_layers: int
    num_heads: int
    intermediate_size: int
    in_channels: int
    image_h: int
    image_w: int
    patch_size: int
    patch_stride: int
    pre_ln: int = 0
    stem_ln: int = 0
    bias_kv: int = 0
    out_dim: int = 1024
    layer_norm_eps: float = 1e-6
    stem_time: int = 1            # > 1: the checkpoint's stem is a Conv3d over this many repeated frames; its kernel is summed over time at load

    @property
    def grid(self) -> Tuple[int, int]:
        return ((self.image_h - self.patch_size) // self.patch_stride + 1, (self.image_w - self.patch_size) // self.patch_stride + 1)

    @property
    def tokens(self) -> int:
        return self.grid[0] * self.grid[1] + 1


@dataclass
class ImageBindConfig:
    vision: ViTTowerConfig = field(default_factory=lambda: ViTTowerConfig(1280, 32, 16, 5120, 3, 224, 224, 14, 14, pre_ln=1, stem_time=2))
    audio: ViTTowerConfig = field(default_factory=lambda: ViTTowerConfig(768, 12, 12, 3072, 1, 128, 204, 16, 10, stem_ln=1, bias_kv=1))
    audio_logit_scale: float = 20.0      # the checkpoint's `log_logit_scale` is not learnable: a constant


def imagebind_huge_config() -> ImageBindConfig:
    return ImageBindConfig()


def imagebind_tiny_config(layers: int = 2) -> ImageBindConfig:
    """the real token geometry (257 / 229 + bias row) at small widths: tests"""
    return ImageBindConfig(vision=ViTTowerConfig(320, layers, 4, 1280, 3, 224, 224, 14, 14, pre_ln=1, stem_time=2),
                           audio=ViTTowerConfig(128, layers, 2, 512, 1, 128, 204, 16, 10, stem_ln=1, bias_kv=1))


# ---- checkpoint keys (`imagebind_huge.pth`: the state dict of the whole six-modality model) --------------------------------------------------------------
def _stem_key(m: str, t: ViTTowerConfig) -> str:
    return f"modality_preprocessors.{m}.rgbt_stem.proj.1.weight" if t.stem_time > 1 else f"modality_preprocessors.{m}.rgbt_stem.proj.weight"


def imagebind_param_specs(cfg: ImageBindConfig, modalities: Sequence[str] = ("vision", "audio")) -> List[Tuple[str, Tuple[int, ...], str]]:
    """(checkpoint key, shape, kind) of the towers asked for; kinds as weights.synthetic_state_dict takes them"""
    s = []
    for m in modalities:
        t: ViTTowerConfig = getattr(cfg, m)
        H, I, p = t.hidden_size, t.intermediate_size, t.patch_size
        pre, tr, hd = f"modality_preprocessors.{m}.", f"modality_trunks.{m}.", f"modality_heads.{m}."
        s += [(pre + "cls_tokens.cls_token", (1, 1, H), "emb"), (pre + "pos_embedding_helper.pos_embed", (1, t.tokens, H), "emb"),
              (_stem_key(m, t), (H, t.in_channels, t.stem_time, p, p) if t.stem_time > 1 else (H, t.in_channels, p, p), "w")]
        if t.stem_ln:
            s += [(pre + "rgbt_stem.norm_layer.weight", (H,), "gamma"), (pre + "rgbt_stem.norm_layer.bias", (H,), "beta")]
        if t.pre_ln:
            s += [(tr + "pre_transformer_layer.0.weight", (H,), "gamma"), (tr + "pre_transformer_layer.0.bias", (H,), "beta")]
        for i in range(t.num_layers):
            b = tr + f"blocks.{i}."
            s += [(b + "attn.in_proj_weight", (3 * H, H), "w"), (b + "attn.in_proj_bias", (3 * H,), "b"),
                  (b + "attn.out_proj.weight", (H, H), "w_res"), (b + "attn.out_proj.bias", (H,), "b")]
            if t.bias_kv:
                s += [(b + "attn.bias_k", (1, 1, H), "emb"), (b + "attn.bias_v", (1, 1, H), "emb")]
            s += [(b + "norm_1.weight", (H,), "gamma"), (b + "norm_1.bias", (H,), "beta"), (b + "norm_2.weight", (H,), "gamma"), (b + "norm_2.bias", (H,), "beta"),
                  (b + "mlp.fc1.weight", (I, H), "w"), (b + "mlp.fc1.bias", (I,), "b"), (b + "mlp.fc2.weight", (H, I), "w_res"), (b + "mlp.fc2.bias", (H,), "b")]
        s += [(hd + "0.weight", (H,), "gamma"), (hd + "0.bias", (H,), "beta"), (hd + "2.weight", (t.out_dim, H), "w")]
    return s


_IGNORED = re.compile(r"^modality_postprocessors\.\w+\.\d+\.log_logit_scale$")


def tower_key(key: str, cfg: ImageBindConfig):
    """checkpoint key -> (modality, key of the tower's `ia2p_vit_load_tensor` or None when the tensor is not read); KeyError for a key of no known form"""
    parts = key.split(".")
    if len(parts) < 3 or parts[0] not in ("modality_preprocessors", "modality_trunks", "modality_heads", "modality_postprocessors"):
        raise KeyError(f"not an ImageBind parameter: '{key}'")
    m, rest = parts[1], ".".join(parts[2:])
    if m in _SKIPPED or _IGNORED.match(key):
        return m, None
    if m not in ("vision", "audio"):
        raise KeyError(f"unknown modality in '{key}'")
    t = getattr(cfg, m)
    if key == _stem_key(m, t):
        return m, "stem.weight"
    table = {"modality_preprocessors": {"cls_tokens.cls_token": "cls_token", "pos_embedding_helper.pos_embed": "pos_embed",
                                        "rgbt_stem.norm_layer.weight": "stem.norm.weight", "rgbt_stem.norm_layer.bias": "stem.norm.bias"},
             "modality_trunks": {"pre_transformer_layer.0.weight": "pre_ln.weight", "pre_transformer_layer.0.bias": "pre_ln.bias"},
             "modality_heads": {"0.weight": "head.norm.weight", "0.bias": "head.norm.bias", "2.weight": "head.proj.weight"}}.get(parts[0], {})
    if rest in table:
        return m, table[rest]
    if parts[0] == "modality_trunks" and parts[2] == "blocks":
        return m, rest              # "blocks.<i>.attn.in_proj_weight", ...: the engine's own names (an unknown one is the engine's KeyError)
    raise KeyError(f"unknown parameter key '{key}'")


class HipViT(_ffi.Executor):
    """one tower behind the C ABI (`ia2p_vit_*`)"""

    def __init__(self, config: ViTTowerConfig, device="cuda:0"):
        self.config = config
        super().__init__("vit", _ffi.make_vit_config(config), device)

    def load_tensor(self, key: str, v: torch.Tensor):
        if key == "stem.weight" and v.ndim == 5:          # Conv3d on a frame repeated along time == Conv2d with the kernel summed over time (fp32 sum, one rounding)
            v = v.detach().float().sum(dim=2)
        super().load_tensor(key, v)

    @torch.no_grad()
    @_ffi.on_device
    def __call__(self, pixels: torch.Tensor, return_hidden: bool = False):
        """pixels [B, C, H, W] -> fp32 [B, out_dim] (head output, not normalised) [, fp16 [B, tokens, hidden]: the last block's output]"""
        cfg = self.config
        if pixels.ndim != 4 or tuple(pixels.shape[1:]) != (cfg.in_channels, cfg.image_h, cfg.image_w):
            raise ValueError(f"expected [B, {cfg.in_channels}, {cfg.image_h}, {cfg.image_w}], got {tuple(pixels.shape)}")
        B = pixels.shape[0]
        x = pixels.to(device=self.device, dtype=torch.float16).contiguous()
        ws = self.workspace(self._lib.ia2p_vit_workspace_bytes(self._h, B))
        out = torch.empty(B, cfg.out_dim, dtype=torch.float32, device=self.device)
        last = torch.empty(B, cfg.tokens, cfg.hidden_size, dtype=torch.float16, device=self.device) if return_hidden else None
        self.check(self._lib.ia2p_vit_encode(self._h, _ffi.current_stream(), _ffi.ptr(x), B, _ffi.ptr(out), _ffi.ptr(last), _ffi.ptr(ws), ws.numel()))
        return (out, last) if return_hidden else out


class HipImageBindModel:
    """`imagebind_huge` restricted to the towers the pipeline calls: `model({'vision': [B,3,224,224]})['vision']` -> L2-normalised fp32 [B,1024];
    `model({'audio': [B,3,1,128,204]})['audio']` -> per clip L2-normalised x 20, averaged over the clips of a file, fp32 [B,1024]."""

    def __init__(self, config: ImageBindConfig = None, device="cuda:0", modalities: Sequence[str] = ("vision", "audio")):
        self.config = config or imagebind_huge_config()
        self.device = torch.device(device)
        for m in modalities:
            if m not in ("vision", "audio"):
                raise ValueError(f"modality '{m}' is not built (vision and audio are)")
        self.modalities = tuple(modalities)
        self.towers: Dict[str, HipViT] = {m: HipViT(getattr(self.config, m), device) for m in self.modalities}

    def eval(self):
        return self

    def to(self, *a, **kw):
        return self

    def load_state_dict(self, state_dict, strict: bool = True):
        """takes the full six-modality dict: tensors of modalities that are not built here are skipped; with strict, an unknown or missing key
        inside a built modality raises KeyError"""
        items = state_dict.items() if hasattr(state_dict, "items") else state_dict
        for k, v in items:
            try:
                m, tk = tower_key(k, self.config)
                if tk is None or m not in self.towers:
                    continue
                self.towers[m].load_tensor(tk, v)
            except KeyError:
                if strict:
                    raise
        for t in self.towers.values():
            try:
                t.finalize()
            except KeyError:
                if strict:
                    raise
        return self

    @torch.no_grad()
    def __call__(self, inputs: dict) -> dict:
        out = {}
        for m, x in inputs.items():
            if m not in self.towers:
                raise ValueError(f"modality '{m}' is not built in this model ({', '.join(self.towers)})")
            if m == "audio":
                if x.ndim != 5:
                    raise ValueError("audio input must be [B, clips, 1, mel bins, frames]")
                B, S = x.shape[:2]
                e = self.towers[m](x.reshape(B * S, *x.shape[2:]))
                e = torch.nn.functional.normalize(e, dim=-1) * self.config.audio_logit_scale
                out[m] = e.reshape(B, S, -1).mean(dim=1)
            else:
                out[m] = torch.nn.functional.normalize(self.towers[m](x), dim=-1)
        return out

    forward = __call__


# ---- host transforms (`imagebind.data`, without torchvision / torchaudio) ---------------------------------------------------------------------------------
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def transform_image(img, size: int = 224) -> torch.Tensor:
    """PIL image (or path) -> fp32 [3, size, size]: RGB, shorter side to `size` (bicubic; long side int(size * long / short)), centre crop, /255, CLIP mean / std"""
    from PIL import Image
    if not isinstance(img, Image.Image):
        with open(img, "rb") as f:
            img = Image.open(f).convert("RGB")
    img = img.convert("RGB")
    w, h = img.size
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    if (nw, nh) != (w, h):
        img = img.resize((nw, nh), Image.BICUBIC)
    top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
    a = np.asarray(img, dtype=np.uint8)[top:top + size, left:left + size].astype(np.float32) / 255.0
    a = (a - np.asarray(CLIP_MEAN, np.float32)) / np.asarray(CLIP_STD, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def load_and_transform_vision_data(image_paths, device):
    if image_paths is None:
        return None
    return torch.stack([transform_image(p) for p in image_paths]).to(device)


def _mel_banks(num_bins: int, fft_len: int, sample_rate: float, low: float, high: float) -> np.ndarray:
    """Kaldi's triangular filters in mel space (mel = 1127 ln(1 + f / 700)): [num_bins, fft_len / 2 + 1], the Nyquist column zero"""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)
    if high <= 0:
        high += sample_rate / 2
    lo, hi = mel(low), mel(high)
    delta = (hi - lo) / (num_bins + 1)
    left = lo + np.arange(num_bins)[:, None] * delta
    m = mel(sample_rate / fft_len * np.arange(fft_len // 2))[None, :]
    banks = np.maximum(0.0, np.minimum((m - left) / delta, (left + 2 * delta - m) / delta))
    return np.pad(banks, ((0, 0), (0, 1)))


def kaldi_fbank(wave: np.ndarray, sample_rate: int = 16000, num_mel_bins: int = 128, frame_length_ms: float = 25.0, frame_shift_ms: float = 10.0,
                preemphasis: float = 0.97, low_freq: float = 20.0, high_freq: float = 0.0) -> np.ndarray:
    """`torchaudio.compliance.kaldi.fbank(htk_compat=True, use_energy=False, window_type='hanning', dither=0.0)` of a mono signal: snip_edges framing,
    per-frame DC removal, pre-emphasis (first sample against itself), symmetric Hann window, FFT padded to a power of two, power spectrum, mel filters,
    natural log floored at fp32 epsilon. -> fp32 [frames, num_mel_bins]"""
    x = np.asarray(wave, np.float64).reshape(-1)
    wl, ws = int(sample_rate * frame_length_ms * 0.001), int(sample_rate * frame_shift_ms * 0.001)
    nfft = 1 << (wl - 1).bit_length()
    if x.size < wl:
        return np.zeros((0, num_mel_bins), np.float32)
    n = 1 + (x.size - wl) // ws
    fr = x[np.arange(n)[:, None] * ws + np.arange(wl)[None, :]]
    fr = fr - fr.mean(axis=1, keepdims=True)
    fr = fr - preemphasis * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(wl) / (wl - 1)))
    power = np.abs(np.fft.rfft(fr, n=nfft, axis=1)) ** 2
    mel = power @ _mel_banks(num_mel_bins, nfft, sample_rate, low_freq, high_freq).T
    return np.log(np.maximum(mel, np.finfo(np.float32).eps)).astype(np.float32)


def clip_timepoints(duration: float, clip_duration: float = 2.0, clips_per_video: int = 3) -> List[Tuple[float, float]]:
    """pytorchvideo's ConstantClipsPerVideoSampler: starts spread evenly over [0, max(duration - clip, 0)]"""
    step = max(duration - clip_duration, 0.0) / max(clips_per_video - 1, 1)
    return [(i * step, i * step + clip_duration) for i in range(clips_per_video)]


def read_wav(path) -> Tuple[np.ndarray, int]:
    """-> (fp32 [channels, samples] in [-1, 1], sample rate); PCM 8 / 16 / 32 bit and IEEE-float WAV"""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    elif data.dtype.kind == "i":
        x = data.astype(np.float32) / float(1 << (8 * data.dtype.itemsize - 1))
    else:
        x = data.astype(np.float32)
    return np.ascontiguousarray(x.reshape(x.shape[0], -1).T), int(sr)


def waveform_to_clips(wave: np.ndarray, sr: int, num_mel_bins: int = 128, target_length: int = 204, sample_rate: int = 16000, clip_duration: float = 2.0,
                      clips_per_video: int = 3, mean: float = -4.268, std: float = 9.138) -> np.ndarray:
    """fp32 [channels, samples] -> fp32 [clips, 1, num_mel_bins, target_length]"""
    if sr != sample_rate:
        from scipy.signal import resample_poly
        g = math.gcd(sr, sample_rate)
        wave = resample_poly(wave, sample_rate // g, sr // g, axis=1).astype(np.float32)
    clips = []
    for t0, t1 in clip_timepoints(wave.shape[1] / sample_rate, clip_duration, clips_per_video):
        c = wave[:, int(t0 * sample_rate):int(t1 * sample_rate)]
        c = c - c.mean()
        fb = kaldi_fbank(c[0], sample_rate, num_mel_bins).T            # [mel bins, frames]
        p = target_length - fb.shape[1]
        fb = np.pad(fb, ((0, 0), (0, p))) if p > 0 else fb[:, :target_length]
        clips.append(((fb - mean) / std)[None])
    return np.stack(clips).astype(np.float32)


def load_and_transform_audio_data(audio_paths, device, num_mel_bins=128, target_length=204, sample_rate=16000, clip_duration=2, clips_per_video=3,
                                  mean=-4.268, std=9.138):
    if audio_paths is None:
        return None
    out = [torch.from_numpy(waveform_to_clips(*read_wav(p), num_mel_bins, target_length, sample_rate, clip_duration, clips_per_video, mean, std)) for p in audio_paths]
    return torch.stack(out).to(device)


def encode_mm_entries(model, kind: str, fnames) -> torch.Tensor:
    """the reference's per-entry branch (pipeline.py:158-164) for all entries of one type as one batch: 'image' | 'audio' files (or PIL images) -> fp32 [n, 1024]"""
    if kind == "audio":
        return model({ModalityType.AUDIO: load_and_transform_audio_data(list(fnames), model.device)})[ModalityType.AUDIO]
    if kind == "image":
        return model({ModalityType.VISION: load_and_transform_vision_data(list(fnames), model.device)})[ModalityType.VISION]
    raise ValueError(f"mm_data entry of type '{kind}': 'image' and 'audio' are encoded")
