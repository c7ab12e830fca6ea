"""The instruction LLM on the HIP kernels and the host plumbing of `forward_llm` (reference instructany2pix/pipeline.py:151-279).

  HipInstructAny2PixLM(config)      <- `InstructAny2PixLMForCausalLM` at inference: a LLaMA decoder (transformers `LlamaForCausalLM`) plus the two
                                       heads of `InstructAny2PixLMMetaModel` the live call uses (llm/model/any2pix_arch.py:38-43):
                                       `vae_projector_image` (1024-d embedding -> hidden) and `vae_predictor_image` (hidden -> embedding)
  .generate(input_ids, ...)         <- `any2pix_lm.generate(...)` as pipeline.py:201-211 calls it. The reference runs one full forward per new
                                       token (`use_cache=False`); here the prompt is prefilled once and each token is one `ia2p_llm_decode`.
  .generate_batch(input_ids_list)   <- several requests at once (no counterpart in the reference): `max_batch` cache slots, each request prefilled
                                       into its own, then one `ia2p_llm_decode_batch` per step reads every weight once for all active requests
  KeywordsStoppingCriteria          <- llm/mm_utils.py:77-107
  vicuna_v1_prompt(inst)            <- `conv_templates['vicuna_v1']` with one user turn and an open assistant turn (llm/conversation.py:51-62,252-262)
  parse_generation(...)             <- pipeline.py:213-279: what `forward_llm` reads out of the generated sequence and its hidden rows

Everything between `inputs_embeds` and (final-normed hidden row, logits row) runs through `ia2p_llm_*`; stopping and the text parsing are host code. The
token is drawn from the logits row on the host (`sampler="host"`, the default: `sample_next` on torch's global RNG) or on the device (`sampler="device"`:
`ia2p_sample_tokens`, one Philox stream per request, the next decode step reading the id from device memory while the host still checks the stopping
criteria). Either sampler takes a nucleus (`top_p=`; `ia2p_sample_tokens_p` on the device), by default the one the checkpoint's generation_config.json names
(`load_generation_config`), else none. The tokenizer is injected (its sentencepiece model is checkpoint data).

Weight format. The reference's live call loads the checkpoint with `load_in_4bit=True, bnb_4bit_compute_dtype=torch.float32` and names no
`bnb_4bit_quant_type` (pipeline.py:28-31). The default of the transformers version it pins (4.34.1) is believed to be "fp4" without double
quantisation; neither that version nor bitsandbytes was at hand to verify it. The unused llm/model/builder.py:31-37 asks for NF4 with double
quantisation. By default this engine computes from the fp16 weights; `load_in_4bit=True` quantises the decoder projections and the two heads
block-wise at load (block 64, fp32 absmax, no double quantisation) with the "fp4" or "nf4" codebook of config.BNB_4BIT_CODEBOOKS, as
bitsandbytes does, and every projection then computes from the dequantised 4-bit weights."""
from __future__ import annotations

import ctypes as C
import re
from types import SimpleNamespace
from typing import Optional

import torch

from . import _ffi
from .config import BNB_4BIT_CODEBOOKS, LLMConfig
from .weights import projector_depth

try:                                  # the protocol `generate(stopping_criteria=[...])` expects; the class works without transformers too
    from transformers import StoppingCriteria as _StoppingCriteria
except Exception:                     # pragma: no cover
    _StoppingCriteria = object


class REPLACEMENT_TYPE:               # reference pipeline.py:89-92
    INPUT = 0
    BASE = 1
    GEN = 2


VICUNA_V1_SYSTEM = ("A chat between a curious user and an artificial intelligence assistant. "
                    "The assistant gives helpful, detailed, and polite answers to the user's questions.")
VICUNA_V1_ROLES = ("USER", "ASSISTANT")
VICUNA_V1_SEP, VICUNA_V1_SEP2 = " ", "</s>"


def vicuna_v1_prompt(inst) -> str:
    """`conv.append_message(USER, inst); conv.append_message(ASSISTANT, None); conv.get_prompt()` under SeparatorStyle.TWO: an empty
    message leaves `role:` without a separator."""
    seps = [VICUNA_V1_SEP, VICUNA_V1_SEP2]
    ret = VICUNA_V1_SYSTEM + seps[0]
    for i, (role, message) in enumerate(((VICUNA_V1_ROLES[0], inst), (VICUNA_V1_ROLES[1], None))):
        if message:
            ret += role + ": " + message + seps[i % 2]
        else:
            ret += role + ":"
    return ret


class KeywordsStoppingCriteria(_StoppingCriteria):
    """llm/mm_utils.py:77-107: stop when the sequence ends in a keyword's ids, or the text decoded from the newest tokens contains a keyword."""

    def __init__(self, keywords, tokenizer, input_ids):
        self.keywords = keywords
        self.keyword_ids = []
        self.max_keyword_len = 0
        for keyword in keywords:
            cur_keyword_ids = tokenizer(keyword).input_ids
            if len(cur_keyword_ids) > 1 and cur_keyword_ids[0] == tokenizer.bos_token_id:
                cur_keyword_ids = cur_keyword_ids[1:]
            if len(cur_keyword_ids) > self.max_keyword_len:
                self.max_keyword_len = len(cur_keyword_ids)
            self.keyword_ids.append(torch.tensor(cur_keyword_ids))
        self.tokenizer = tokenizer
        self.start_len = input_ids.shape[1]

    def call_bse(self, output_ids, scores, **kwargs) -> bool:
        assert output_ids.shape[0] == 1, "Only support batch size 1 (yet)"
        offset = min(output_ids.shape[1] - self.start_len, self.max_keyword_len)
        self.keyword_ids = [keyword_id.to(output_ids.device) for keyword_id in self.keyword_ids]
        for keyword_id in self.keyword_ids:
            tail = output_ids[0, -keyword_id.shape[0]:]
            if tail.shape[0] == keyword_id.shape[0] and (tail == keyword_id).all():
                return True
        outputs = self.tokenizer.batch_decode(output_ids[:, -offset:], skip_special_tokens=True)[0]
        for keyword in self.keywords:
            if keyword in outputs:
                return True
        return False

    def __call__(self, output_ids, scores, **kwargs) -> bool:
        return all(self.call_bse(output_ids[i:i + 1], scores=None, **kwargs) for i in range(output_ids.shape[0]))


def _check_top_p(top_p) -> float:
    """`TopPLogitsWarper.__init__`'s check and wording; NaN and 0 are refused too (the device sampler refuses them, and a nucleus of mass 0 names no token)"""
    try:
        p = float(top_p)
    except (TypeError, ValueError):
        p = float("nan")
    if not (0.0 < p <= 1.0):
        raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
    return p


def _check_top_k(top_k):
    """None and 0 switch top-k off (as `generate` reads them); anything else is `TopKLogitsWarper.__init__`'s check and wording"""
    if top_k is None or (isinstance(top_k, int) and not isinstance(top_k, bool) and top_k == 0):
        return None
    if not isinstance(top_k, int) or isinstance(top_k, bool) or top_k <= 0:
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {top_k}")
    return top_k


def sample_probs(logits: torch.Tensor, temperature: float = 0.3, top_k: Optional[int] = 50, top_p: float = 1.0) -> torch.Tensor:
    """The distribution transformers' sampling loop draws from: `TemperatureLogitsWarper` -> `TopKLogitsWarper` -> `TopPLogitsWarper` -> softmax, in that
    order. (transformers 4.34.1, which the reference pins, carries `top_k=50, top_p=1.0` in its default generation config; `generate` starts from the
    checkpoint's own generation_config.json, and adds the top-p warper only when that holds `top_p < 1`: at `top_p >= 1` nothing is sorted here either.)
    The top-p step is `TopPLogitsWarper.__call__` restated: sort ascending, remove while the cumulative probability is <= 1 - top_p, never the last.
    logits: [..., vocab] fp32."""
    top_p = _check_top_p(top_p)
    scores = logits.float() / temperature
    if top_k is not None and top_k > 0:
        k = min(int(top_k), scores.shape[-1])
        scores = scores.masked_fill(scores < torch.topk(scores, k)[0][..., -1, None], -float("inf"))
    if top_p < 1.0:
        sorted_scores, sorted_indices = torch.sort(scores, descending=False)
        remove = sorted_scores.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        remove[..., -1:] = False                          # min_tokens_to_keep = 1
        scores = scores.masked_fill(remove.scatter(-1, sorted_indices, remove), -float("inf"))
    return torch.nn.functional.softmax(scores, dim=-1)


def sample_next(logits: torch.Tensor, do_sample: bool = True, temperature: float = 0.3, top_k: Optional[int] = 50, top_p: float = 1.0) -> torch.Tensor:
    """[1, vocab] logits -> [1] token ids; `torch.multinomial` on the global RNG of the logits' device, or argmax."""
    if not do_sample:
        return torch.argmax(logits, dim=-1)
    return torch.multinomial(sample_probs(logits, temperature, top_k, top_p), num_samples=1).squeeze(1)


GENERATION_CONFIG_NAME = "generation_config.json"
GENERATION_DEFAULTS = {"top_k": 50, "top_p": 1.0}          # transformers' default generation config, as far as this sampler reads it


def read_generation_config(path_or_dict) -> dict:
    """A generation_config.json (a dict with its content, the file, or a checkpoint folder that holds one) -> the keys this sampler reads, `top_k`,
    `top_p` and `temperature`, checked; every other key is ignored, a key the file does not carry is not in the result."""
    import json
    import os
    cfg = path_or_dict
    if not isinstance(cfg, dict):
        path = os.fspath(cfg)
        if os.path.isdir(path):
            path = os.path.join(path, GENERATION_CONFIG_NAME)
        with open(path) as f:
            cfg = json.load(f)
        if not isinstance(cfg, dict):
            raise ValueError(f"{path}: a generation config is a JSON object")
    out = {}
    if cfg.get("top_p") is not None:
        out["top_p"] = _check_top_p(cfg["top_p"])
    if "top_k" in cfg:
        out["top_k"] = _check_top_k(cfg["top_k"])
    if cfg.get("temperature") is not None:
        t = cfg["temperature"]
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t > 0 and t < float("inf")):
            raise ValueError(f"`temperature` has to be a strictly positive float, but is {t}")
        out["temperature"] = float(t)
    return out


SAMPLERS = ("host", "device")


def _resolve_sampler(sampler, default=None):
    """the `sampler` argument of the constructor and of `generate` / `generate_batch` (None there: the constructor's choice)"""
    if sampler is None and default is not None:
        return default
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler {sampler!r}: one of {SAMPLERS}")
    return sampler


def _resolve_seeds(seeds, n_req):
    """one Philox key per request: the given ones, or 63-bit draws from torch's global CPU generator in request order (`torch.manual_seed` fixes a run)"""
    if seeds is None:
        return [int(torch.randint(0, 2 ** 63 - 1, (1,)).item()) for _ in range(n_req)]
    seeds = [int(s) for s in seeds]
    if len(seeds) != n_req:
        raise ValueError(f"{len(seeds)} seeds for {n_req} requests: one per request")
    if any(s < 0 or s >= 2 ** 64 for s in seeds):
        raise ValueError("a seed is a 64-bit unsigned integer")
    return seeds


class _LastOnly(tuple):
    """`hidden_states[i]` of the output object: only [-1] is materialised, and of it only the last position (all the reference reads:
    `output_ids.hidden_states[i][-1][:, -1:]`, pipeline.py:236,242,257)."""

    def __new__(cls, h, n):
        t = super().__new__(cls, (h,))
        t._n = n
        return t

    def __getitem__(self, i):
        if i in (-1, self._n - 1):
            return tuple.__getitem__(self, 0)
        raise IndexError("only hidden_states[i][-1] (its last position) is computed on the HIP path")

    def __len__(self):
        return self._n


class _Head:
    """`nn.Linear` or `mlpNx_gelu` Sequential of Linears (builder.py:33-74) on ia2p_linear_small (+ ia2p_gelu between the linears)."""

    def __init__(self, name, depth):
        self.name, self.depth = name, depth
        self.w, self.b = [None] * depth, [None] * depth

    def key_slot(self, key):
        rest = key[len(self.name) + 1:]
        if self.depth == 1 and rest in ("weight", "bias"):
            return 0, rest
        m = re.match(r"^(\d+)\.(weight|bias)$", rest)
        if not m or int(m.group(1)) % 2 or int(m.group(1)) // 2 >= self.depth:
            raise KeyError(f"unknown parameter key '{key}'")
        return int(m.group(1)) // 2, m.group(2)

    def load(self, key, t):
        j, what = self.key_slot(key)
        (self.w if what == "weight" else self.b)[j] = t

    def missing(self):
        return [f"{self.name}[{j}]" for j in range(self.depth) if self.w[j] is None or self.b[j] is None]

    def __call__(self, lib, x):
        lead = x.shape[:-1]
        h = x.reshape(-1, x.shape[-1]).to(device=self.w[0].device, dtype=torch.float16).contiguous()
        for j in range(self.depth):
            N, K = self.w[j].shape
            if h.shape[1] != K:
                raise ValueError(f"{self.name}: input width {h.shape[1]}, expected {K}")
            out = torch.empty(h.shape[0], N, dtype=torch.float16, device=h.device)
            for r0 in range(0, h.shape[0], 16):
                rows = min(16, h.shape[0] - r0)
                _ffi.check(lib.ia2p_linear_small(_ffi.current_stream(), _ffi.ptr(h[r0:r0 + rows]), _ffi.ptr(self.w[j]), _ffi.ptr(self.b[j]),
                                                 _ffi.ptr(out[r0:r0 + rows]), rows, N, K, 0, 0))
            if j < self.depth - 1 and out.numel():
                _ffi.check(lib.ia2p_gelu(_ffi.current_stream(), _ffi.ptr(out), out.numel()))
            h = out
        return h.float().reshape(*lead, h.shape[-1])


class HipInstructAny2PixLM(_ffi.Executor):
    PROJECTOR, PREDICTOR = "model.vae_projector_image", "model.vae_predictor_image"

    MAX_ROWS = 8                       # IA2P_LLM_MAX_ROWS: sequences per decode_batch call
    sampler = "host"                   # the constructor sets it per instance; the class default serves subclasses that stand in for the engine without
                                       # running the constructor (tests/test_llm_batch_cpu.py drives `generate_batch` through one)
    generation_defaults = dict(GENERATION_DEFAULTS)      # likewise: the constructor gives the instance its own copy, `load_generation_config` a new one

    def __init__(self, config: LLMConfig, device="cuda:0", max_positions: int = 1024, video_token_id: Optional[int] = None, *,
                 load_in_4bit: bool = False, bnb_4bit_quant_type: str = "fp4", quantize_heads: bool = True, max_batch: int = 1, sampler: str = "host"):
        """sampler: where `generate` / `generate_batch` draw the next token, "host" (torch on the CPU, from a copy of the logits row) or "device"
        (`ia2p_sample_tokens` on the row where it lies); either call takes `sampler=` to override it. max_batch: cache slots, i.e. requests `generate_batch` decodes together (a slot holds `max_positions` rows of every layer: 512 MiB
        at Vicuna-7B size and 1024 positions; the default keeps the single-sequence memory). load_in_4bit / bnb_4bit_quant_type: the reference's `from_pretrained` keywords. quantize_heads: the two projector heads are
        `nn.Linear`s inside the model, so the reference's loader quantises them with the decoder (it skips `lm_head` only); False keeps
        their fp16 weights."""
        if bnb_4bit_quant_type not in BNB_4BIT_CODEBOOKS:
            raise ValueError(f"bnb_4bit_quant_type '{bnb_4bit_quant_type}': one of {sorted(BNB_4BIT_CODEBOOKS)}")
        if max_batch < 1:
            raise ValueError(f"max_batch {max_batch}: at least one slot")
        self.sampler = _resolve_sampler(sampler)
        self.generation_defaults = dict(GENERATION_DEFAULTS)
        self.config = config.validate()
        self.max_positions = max_positions
        self.max_batch = int(max_batch)
        self.DEFAULT_VIDEO_TOKEN_IDX = video_token_id        # id of `<video>` (set by the tokenizer side, any2pix_arch.py:285-288)
        self.quant_type = bnb_4bit_quant_type if load_in_4bit else None
        self._codebook = (C.c_float * 16)(*BNB_4BIT_CODEBOOKS[bnb_4bit_quant_type])
        self._quantize_heads = bool(load_in_4bit and quantize_heads)

        def weight_format():               # decides the arena's layout: before the arena is sized
            if load_in_4bit:
                self.check(self._lib.ia2p_llm_set_weight_format(self._h, 4, self._codebook))

        super().__init__("llm", _ffi.make_llm_config(config), device, prepare=weight_format)
        with self._on_device():
            self.kv = torch.zeros(self._lib.ia2p_llm_kv_slots_bytes(self._h, max_positions, self.max_batch), dtype=torch.uint8, device=self.device)
        self.check(self._lib.ia2p_llm_bind_kv_slots(self._h, _ffi.ptr(self.kv), self.kv.numel(), max_positions, self.max_batch))
        d = projector_depth(config.mm_projector_type)
        self._projector, self._predictor = _Head(self.PROJECTOR, d), _Head(self.PREDICTOR, d)
        self._ws_T = 0
        self._tok_dev = self._tok_host = None              # device sampler: the drawn ids on the device and their pinned host copy
        self.dtype = torch.float16

    def get_model(self):               # `any2pix_lm.get_model().vae_predictor_image(...)` (pipeline.py:236)
        return self

    @property
    def weight_bits(self) -> int:
        """16, or 4 when the decoder projections are held as 4-bit codes"""
        return self._lib.ia2p_llm_weight_bits(self._h)

    @_ffi.on_device
    def _quantize_round_trip(self, key, w):
        """fp16 [N, K] -> the fp16 weights bitsandbytes' Linear4bit computes from: quantised block-wise and dequantised once"""
        N, K = w.shape
        if w.numel() % 64:
            raise ValueError(f"'{key}': {w.numel()} weights do not divide into blocks of 64")
        rows, cols = w.numel() // 64, 64          # blocks run along the flattened tensor
        packed = torch.empty(self._lib.ia2p_llm_q4_packed_bytes(rows, cols), dtype=torch.uint8, device=w.device)
        absmax = torch.empty(rows, dtype=torch.float32, device=w.device)
        out = torch.empty_like(w)
        s = _ffi.current_stream()
        _ffi.check(self._lib.ia2p_llm_quantize_q4(s, _ffi.ptr(w), rows, cols, self._codebook, _ffi.ptr(packed), _ffi.ptr(absmax)), None, "llm")
        _ffi.check(self._lib.ia2p_llm_dequantize_q4(s, _ffi.ptr(packed), _ffi.ptr(absmax), rows, cols, self._codebook, _ffi.ptr(out)), None, "llm")
        torch.cuda.current_stream().synchronize()
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        items = state_dict.items() if hasattr(state_dict, "items") else state_dict
        for k, v in items:
            if k.endswith("rotary_emb.inv_freq"):          # buffer in older transformers checkpoints
                continue
            if k.startswith((self.PROJECTOR + ".", self.PREDICTOR + ".")):      # the heads live in torch tensors of their own, not in the arena
                t = v.detach().to(device=self.device, dtype=torch.float16).contiguous()
                if self._quantize_heads and k.endswith(".weight"):
                    t = self._quantize_round_trip(k, t)
                (self._projector if k.startswith(self.PROJECTOR + ".") else self._predictor).load(k, t)
            else:
                self.load_tensor(k, v)
        if strict:
            missing = self._projector.missing() + self._predictor.missing()
            if missing:
                raise KeyError(f"projector head parameters not loaded: {missing}")
            self.finalize()

    # ---- the two heads -----------------------------------------------------------------------------------------------
    @_ffi.on_device
    def vae_projector_image(self, x):
        return self._projector(self._lib, x)

    @_ffi.on_device
    def vae_predictor_image(self, x):
        return self._predictor(self._lib, x)

    # ---- engine calls ---------------------------------------------------------------------------------------------------
    def _workspace(self, T):
        if self._ws is None or T > self._ws_T:
            self.workspace(self._lib.ia2p_llm_batch_workspace_bytes(self._h, T, min(self.max_batch, self.MAX_ROWS)))
            self._ws_T = T
        return self._ws

    def reset(self):
        self.check(self._lib.ia2p_llm_reset(self._h))

    @property
    def position(self) -> int:
        return self._lib.ia2p_llm_position(self._h)

    @_ffi.on_device
    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        ids = ids.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty(ids.numel(), self.config.hidden_size, dtype=torch.float16, device=self.device)
        self.check(self._lib.ia2p_llm_embed(self._h, _ffi.current_stream(), _ffi.ptr(ids), ids.numel(), _ffi.ptr(out)))
        return out

    def _outputs(self):
        return (torch.empty(self.config.hidden_size, dtype=torch.float32, device=self.device),
                torch.empty(self.config.vocab_size, dtype=torch.float32, device=self.device))

    @torch.no_grad()
    @_ffi.on_device
    def prefill(self, inputs_embeds: torch.Tensor):
        """[T, hidden] rows at the current position -> (final-normed hidden row [hidden], logits row [vocab]) of the last one, fp32"""
        x = inputs_embeds.to(device=self.device, dtype=torch.float16).contiguous()
        if x.ndim != 2 or x.shape[1] != self.config.hidden_size:
            raise ValueError("inputs_embeds must be [T, hidden]")
        ws = self._workspace(x.shape[0])
        hid, logits = self._outputs()
        self.check(self._lib.ia2p_llm_prefill(self._h, _ffi.current_stream(), _ffi.ptr(x), x.shape[0], _ffi.ptr(hid), _ffi.ptr(logits),
                                               _ffi.ptr(ws), ws.numel()))
        return hid, logits

    @torch.no_grad()
    @_ffi.on_device
    def decode(self, token_id: int):
        """one row (the table embedding of token_id) at the current position -> (hidden row, logits row), fp32"""
        ws = self._workspace(max(self._ws_T, 1))
        hid, logits = self._outputs()
        self.check(self._lib.ia2p_llm_decode(self._h, _ffi.current_stream(), int(token_id), _ffi.ptr(hid), _ffi.ptr(logits), _ffi.ptr(ws), ws.numel()))
        return hid, logits

    # ---- slots: several sequences in one cache ------------------------------------------------------------------------------
    def reset_slot(self, slot: int):
        self.check(self._lib.ia2p_llm_reset_slot(self._h, int(slot)))

    def slot_position(self, slot: int) -> int:
        return self._lib.ia2p_llm_slot_position(self._h, int(slot))

    @torch.no_grad()
    @_ffi.on_device
    def prefill_slot(self, slot: int, inputs_embeds: torch.Tensor):
        """`prefill` on the cache and position of `slot`; the other slots are not touched"""
        x = inputs_embeds.to(device=self.device, dtype=torch.float16).contiguous()
        if x.ndim != 2 or x.shape[1] != self.config.hidden_size:
            raise ValueError("inputs_embeds must be [T, hidden]")
        ws = self._workspace(x.shape[0])
        hid, logits = self._outputs()
        self.check(self._lib.ia2p_llm_prefill_slot(self._h, _ffi.current_stream(), int(slot), _ffi.ptr(x), x.shape[0], _ffi.ptr(hid), _ffi.ptr(logits),
                                                    _ffi.ptr(ws), ws.numel()))
        return hid, logits

    @torch.no_grad()
    @_ffi.on_device
    def decode_batch(self, slots, token_ids):
        """one decode step of the sequences in `slots` (distinct, at most 8): row r is the table embedding of token_ids[r] at the position of
        slots[r] -> (hidden rows [n, hidden], logits rows [n, vocab]), fp32; every weight is read once for all rows"""
        slots, token_ids = [int(s) for s in slots], [int(t) for t in token_ids]
        if len(slots) != len(token_ids):
            raise ValueError(f"{len(slots)} slots for {len(token_ids)} token ids")
        n = len(slots)
        ws = self._workspace(max(self._ws_T, 1))
        hid = torch.empty(max(n, 1), self.config.hidden_size, dtype=torch.float32, device=self.device)
        logits = torch.empty(max(n, 1), self.config.vocab_size, dtype=torch.float32, device=self.device)
        ids = C.c_int32 * max(n, 1)
        self.check(self._lib.ia2p_llm_decode_batch(self._h, _ffi.current_stream(), ids(*slots), ids(*token_ids), n, _ffi.ptr(hid), _ffi.ptr(logits),
                                                    _ffi.ptr(ws), ws.numel()))
        return hid, logits

    @torch.no_grad()
    @_ffi.on_device
    def decode_batch_dev(self, slots, dev_tokens: torch.Tensor, token_index=None):
        """`decode_batch` with the ids in device memory: row r embeds dev_tokens[token_index[r]] (dev_tokens: int32 on the device, token_index: host
        indices into it, None = 0..n-1). The host never reads the ids; an id outside the vocabulary is clamped into the table by the kernel."""
        slots = [int(s) for s in slots]
        n = len(slots)
        index = list(range(n)) if token_index is None else [int(t) for t in token_index]
        if len(index) != n:
            raise ValueError(f"{n} slots for {len(index)} token indices")
        if dev_tokens.dtype != torch.int32 or dev_tokens.device != self.device or (index and max(index) >= dev_tokens.numel()):
            raise ValueError(f"dev_tokens must be int32 on {self.device} and hold every index of token_index")
        ws = self._workspace(max(self._ws_T, 1))
        hid = torch.empty(max(n, 1), self.config.hidden_size, dtype=torch.float32, device=self.device)
        logits = torch.empty(max(n, 1), self.config.vocab_size, dtype=torch.float32, device=self.device)
        ids = C.c_int32 * max(n, 1)
        self.check(self._lib.ia2p_llm_decode_batch_dev(self._h, _ffi.current_stream(), ids(*slots), _ffi.ptr(dev_tokens), ids(*index), n, _ffi.ptr(hid),
                                                        _ffi.ptr(logits), _ffi.ptr(ws), ws.numel()))
        return hid, logits

    def load_generation_config(self, path_or_dict) -> dict:
        """What `from_pretrained` does with the checkpoint's generation_config.json: its `top_k`, `top_p` and `temperature` (a dict, the file, or the
        checkpoint folder; other keys are ignored, an invalid value raises ValueError and changes nothing) replace the entries of
        `generation_defaults`. `generate` / `generate_batch` read `top_p` from there when the call passes none. Their `top_k` and `temperature` keywords carry
        defaults of their own (50, 0.3: the reference passes the temperature explicitly), which a call that names neither still gets; the loaded
        values stand in `generation_defaults` for a caller to pass on. -> the new `generation_defaults`."""
        self.generation_defaults = {**self.generation_defaults, **read_generation_config(path_or_dict)}
        return self.generation_defaults

    def _resolve_top_p(self, top_p) -> float:
        """the `top_p` keyword: the call's own value, else the loaded generation config's, else 1.0; checked before any device work"""
        return _check_top_p(self.generation_defaults.get("top_p", 1.0) if top_p is None else top_p)

    def sample_tokens(self, logits: torch.Tensor, seeds, steps, do_sample: bool = True, temperature: float = 0.3, top_k: Optional[int] = 50, out=None,
                      top_p: Optional[float] = None):
        """`ia2p_sample_tokens_p` on the fp32 rows [n, vocab] of `logits` (device): row r drawn with key seeds[r] at counter steps[r] -> int32 [n] on the
        device (`out`, or a new tensor). top_p None: `generation_defaults`' (1.0 unless a generation config was loaded; at 1.0 the launch is
        `ia2p_sample_tokens`'s). Nothing is synchronised."""
        top_p = self._resolve_top_p(top_p)
        block = logits.reshape(-1, logits.shape[-1])
        if block.dtype != torch.float32 or block.stride(1) != 1:
            raise ValueError("logits must be fp32 rows")
        n, V = block.shape
        if len(seeds) != n or len(steps) != n:
            raise ValueError(f"{n} rows, {len(seeds)} seeds, {len(steps)} steps")
        out = torch.empty(n, dtype=torch.int32, device=block.device) if out is None else out[:n]
        with self._on_device():            # (behind the argument checks: they need no engine)
            _ffi.check(self._lib.ia2p_sample_tokens_p(_ffi.current_stream(), C.c_void_p(block.data_ptr()), block.stride(0) if n > 1 else V, n, V, float(temperature),
                                                      int(top_k or 0), top_p, int(bool(do_sample)), (C.c_uint64 * n)(*seeds), (C.c_uint32 * n)(*steps), _ffi.ptr(out),
                                                      None, None), None, "llm")
        return out

    def prepare_inputs_embeds(self, input_ids: torch.Tensor, extra_replacement=None) -> torch.Tensor:
        """`embed_tokens(input_ids)` with the modality vectors at the `<video>` positions, as any2pix_llama.py:277-291 builds them at
        inference: with n = len(mask), the first n `<video>` positions are candidates (`a[:n]`, `b[:n]`), those whose mask entry is INPUT
        receive `vae_projector_image(data[mask == INPUT])` in order. The reference ADDS the projection to the table embedding of `<video>`:
        its line 289 zeroes a temporary (chained advanced indexing returns a copy), so `z + inputs_embeds` keeps the table row. Later
        `<video>` positions -- generated ones included -- keep their table embedding alone."""
        ids = input_ids.reshape(-1)
        emb = self.embed_tokens(ids)
        if extra_replacement is None:
            return emb
        if self.DEFAULT_VIDEO_TOKEN_IDX is None:
            raise ValueError("extra_replacement needs video_token_id (the id of `<video>`)")
        mask = torch.as_tensor(extra_replacement["mask"]).reshape(-1).cpu()
        n = mask.shape[0]
        pos = torch.where(ids.cpu() == self.DEFAULT_VIDEO_TOKEN_IDX)[0][:n]
        if pos.shape[0] != n:
            raise ValueError(f"{n} replacement entries for {pos.shape[0]} `<video>` tokens in the prompt")
        sel = mask == REPLACEMENT_TYPE.INPUT
        if sel.any():
            z2 = self.vae_projector_image(torch.as_tensor(extra_replacement["data"])[sel])
            rows = pos[sel].to(self.device)
            emb[rows] = (emb[rows].float() + z2).to(torch.float16)
        return emb

    @torch.no_grad()
    def generate(self, input_ids, extra_replacement=None, do_sample: bool = True, temperature: float = 0.3, max_new_tokens: int = 100,
                 stopping_criteria=None, top_k: Optional[int] = 50, sampler: Optional[str] = None, seed: Optional[int] = None, top_p: Optional[float] = None,
                 **unused):
        """-> object with `.sequences` ([1, prompt + new] on the host) and `.hidden_states` (one entry per new token;
        `hidden_states[i][-1][:, -1:]` is step i's final-normed last-position row, [1, 1, hidden] fp32 on the device).
        sampler: "host" or "device" (None: the constructor's). seed ("device" only): the request's Philox key; None draws one from torch's global CPU
        generator. The tokens of a seed are those the request gets inside any `generate_batch(sampler="device")` call under the same seed. Under "host"
        `seed` is not used: that path draws from torch's global RNG, as it always has. top_p: the nucleus of either sampler; None takes
        `generation_defaults["top_p"]` (what `load_generation_config` read, else 1.0: no nucleus, the path this call has always taken)."""
        sampler = _resolve_sampler(sampler, self.sampler)
        top_p = self._resolve_top_p(top_p)
        if input_ids.ndim != 2 or input_ids.shape[0] != 1:
            raise ValueError("input_ids must be [1, tokens] (batch 1, as the reference asserts)")
        if sampler == "device":
            return self._generate_device([input_ids], [extra_replacement], do_sample, temperature, max_new_tokens, [stopping_criteria], top_k,
                                         None if seed is None else [seed], top_p)[0]
        seq = input_ids.detach().cpu().long()
        T = seq.shape[1]
        if T + max_new_tokens > self.max_positions:
            raise ValueError(f"{T} prompt tokens + {max_new_tokens} new ones do not fit {self.max_positions} cached positions")
        emb = self.prepare_inputs_embeds(seq, extra_replacement)
        self.reset()
        hid, logits = self.prefill(emb)
        nl = self.config.num_hidden_layers + 1
        hidden_states = []
        for step in range(max_new_tokens):
            hidden_states.append(_LastOnly(hid.reshape(1, 1, -1), nl))
            nxt = sample_next(logits.reshape(1, -1).cpu(), do_sample, temperature, top_k, top_p)
            seq = torch.cat([seq, nxt.reshape(1, 1).long()], dim=1)
            if stopping_criteria is not None and any(bool(torch.as_tensor(c(seq, None)).all()) for c in stopping_criteria):
                break
            if step + 1 < max_new_tokens:
                hid, logits = self.decode(int(nxt))
        return SimpleNamespace(sequences=seq, hidden_states=tuple(hidden_states))


    @torch.no_grad()
    def generate_batch(self, input_ids_list, extra_replacements=None, do_sample: bool = True, temperature: float = 0.3, max_new_tokens: int = 100,
                       stopping_criteria=None, top_k: Optional[int] = 50, sampler: Optional[str] = None, seeds=None, top_p: Optional[float] = None, **unused):
        """`generate` for several requests. input_ids_list: [1, T_i] prompts; extra_replacements / stopping_criteria: one entry per request (an
        `extra_replacement` dict / a list of criteria, or None), or None. -> a list with one `generate`-shaped object per request
        (`.sequences` [1, T_i + new_i], `.hidden_states` with one entry per new token).

        Requests run in consecutive groups of `max_batch`, at most 8 to a group. Each request of a group is prefilled into its own slot, then every
        step brings the active rows' logits to the host in one copy, draws one token per row and decodes the rows that go on in one
        `decode_batch` call; a request that stops, or has `max_new_tokens`, leaves the active set and the later calls carry fewer rows.
        Each request's stopping criteria see that request's sequence only.

        do_sample=False gives exactly the sequences and hidden rows of serial `generate(do_sample=False)` calls (a row of `decode_batch` equals
        the single-sequence step bit for bit). do_sample=True draws all active rows of a step with ONE `torch.multinomial` call over the
        [n_active, vocab] block, in request order: the draws of the requests interleave in the global RNG stream, so a batch is reproducible
        for a seed but is not the stream serial `generate` calls would consume.

        sampler="device" (None: the constructor's choice) draws on the device instead, request i from its own Philox stream keyed by seeds[i] (None: one
        63-bit seed per request from torch's global CPU generator): each request then gets exactly the tokens and hidden rows of
        `generate(sampler="device", seed=seeds[i])`, whatever shares its batch. See `_generate_device`. Under "host" `seeds` is checked for its length
        and otherwise not used: that path draws from torch's global RNG, as it always has. top_p: as in `generate`."""
        sampler = _resolve_sampler(sampler, self.sampler)
        top_p = self._resolve_top_p(top_p)
        prompts = list(input_ids_list)
        n_req = len(prompts)
        seeds = None if seeds is None else list(seeds)
        if seeds is not None and len(seeds) != n_req:
            raise ValueError(f"{len(seeds)} seeds for {n_req} requests: one per request")
        if sampler == "device":
            return self._generate_device(prompts, extra_replacements, do_sample, temperature, max_new_tokens, stopping_criteria, top_k, seeds, top_p)
        reps = list(extra_replacements) if extra_replacements is not None else [None] * n_req
        crits = list(stopping_criteria) if stopping_criteria is not None else [None] * n_req
        if len(reps) != n_req or len(crits) != n_req:
            raise ValueError(f"{n_req} prompts, {len(reps)} extra_replacements, {len(crits)} stopping_criteria: one entry per request")
        seqs = []
        for p in prompts:
            if p.ndim != 2 or p.shape[0] != 1:
                raise ValueError("every prompt must be [1, tokens]")
            if p.shape[1] + max_new_tokens > self.max_positions:
                raise ValueError(f"{p.shape[1]} prompt tokens + {max_new_tokens} new ones do not fit {self.max_positions} cached positions")
            seqs.append(p.detach().cpu().long())
        nl = self.config.num_hidden_layers + 1
        hidden = [[] for _ in range(n_req)]
        group = min(self.max_batch, self.MAX_ROWS)
        for g0 in range(0, n_req, group):
            active = list(range(g0, min(g0 + group, n_req)))             # request i of the group lives in slot i - g0
            rows = []
            for i in active:
                self.reset_slot(i - g0)
                rows.append(self.prefill_slot(i - g0, self.prepare_inputs_embeds(seqs[i], reps[i])))
            hid, logits = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])
            for step in range(max_new_tokens):
                for r, i in enumerate(active):
                    hidden[i].append(_LastOnly(hid[r].reshape(1, 1, -1), nl))
                block = logits.cpu()                                     # [n_active, vocab]: one copy per step
                if do_sample:
                    nxt = torch.multinomial(sample_probs(block, temperature, top_k, top_p), num_samples=1).squeeze(1)
                else:
                    nxt = torch.argmax(block, dim=-1)
                go_on, tokens = [], []
                for r, i in enumerate(active):
                    seqs[i] = torch.cat([seqs[i], nxt[r].reshape(1, 1).long()], dim=1)
                    if crits[i] is not None and any(bool(torch.as_tensor(c(seqs[i], None)).all()) for c in crits[i]):
                        continue
                    go_on.append(i)
                    tokens.append(int(nxt[r]))
                active = go_on
                if not active or step + 1 == max_new_tokens:
                    break
                hid, logits = self.decode_batch([i - g0 for i in active], tokens)
        return [SimpleNamespace(sequences=seqs[i], hidden_states=tuple(hidden[i])) for i in range(n_req)]


    @torch.no_grad()
    @_ffi.on_device
    def _generate_device(self, prompts, extra_replacements, do_sample, temperature, max_new_tokens, stopping_criteria, top_k, seeds, top_p: Optional[float] = None):
        """`generate_batch` with the token drawn on the device. Per step of a group: `ia2p_sample_tokens_p` on the step's logits block, the ids copied
        asynchronously into pinned host memory, an event behind the copy, and -- before the host waits for that event -- the next `decode_batch_dev`
        for every row still active, reading its id from device memory. Only then are the ids read, appended and shown to the stopping criteria. A
        request that turns out to have stopped has had one decode row too many computed: that row is dropped (it is never appended to
        `hidden_states`, and the slot is reset at its next use), and from the next step on `token_index` names the live rows of the id buffer.
        Row r of a step is drawn under (seed of its request, number of tokens the request has): nothing depends on the other rows."""
        n_req = len(prompts)
        top_p = self._resolve_top_p(top_p)
        reps = list(extra_replacements) if extra_replacements is not None else [None] * n_req
        crits = list(stopping_criteria) if stopping_criteria is not None else [None] * n_req
        if len(reps) != n_req or len(crits) != n_req:
            raise ValueError(f"{n_req} prompts, {len(reps)} extra_replacements, {len(crits)} stopping_criteria: one entry per request")
        seeds = _resolve_seeds(seeds, n_req) if do_sample or seeds is not None else [0] * n_req      # (argmax consumes no random numbers)
        seqs = []
        for p in prompts:
            if p.ndim != 2 or p.shape[0] != 1:
                raise ValueError("every prompt must be [1, tokens]")
            if p.shape[1] + max_new_tokens > self.max_positions:
                raise ValueError(f"{p.shape[1]} prompt tokens + {max_new_tokens} new ones do not fit {self.max_positions} cached positions")
            seqs.append(p.detach().cpu().long())
        if self._tok_dev is None:
            self._tok_dev = torch.zeros(self.MAX_ROWS, dtype=torch.int32, device=self.device)
            self._tok_host = torch.zeros(self.MAX_ROWS, dtype=torch.int32).pin_memory()
        nl = self.config.num_hidden_layers + 1
        hidden = [[] for _ in range(n_req)]
        group = min(self.max_batch, self.MAX_ROWS)
        for g0 in range(0, n_req, group):
            block = list(range(g0, min(g0 + group, n_req)))              # the requests behind the rows of `logits`; request i lives in slot i - g0
            rows = []
            for i in block:
                self.reset_slot(i - g0)
                rows.append(self.prefill_slot(i - g0, self.prepare_inputs_embeds(seqs[i], reps[i])))
            hid, logits = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])
            active = list(block)                                         # the requests that have not stopped: a subset of `block`, in its order
            for step in range(max_new_tokens):
                for i in active:
                    hidden[i].append(_LastOnly(hid[block.index(i)].reshape(1, 1, -1), nl))
                self.sample_tokens(logits, [seeds[i] for i in block], [step] * len(block), do_sample, temperature, top_k, out=self._tok_dev, top_p=top_p)
                self._tok_host[:len(block)].copy_(self._tok_dev[:len(block)], non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                drawn_for = block
                if step + 1 < max_new_tokens:                            # one step ahead: every active row, before the host knows which of them stop
                    hid, logits = self.decode_batch_dev([i - g0 for i in active], self._tok_dev, [block.index(i) for i in active])
                    block = active
                done.synchronize()
                tokens = self._tok_host[:len(drawn_for)].tolist()
                go_on = []
                for i in active:
                    t = tokens[drawn_for.index(i)]
                    if t < 0:
                        raise RuntimeError(f"request {i}: the logits of step {step} hold NaN or +inf, or nothing finite (no token can be drawn)")
                    seqs[i] = torch.cat([seqs[i], torch.tensor([[t]], dtype=torch.long)], dim=1)
                    if crits[i] is not None and any(bool(torch.as_tensor(c(seqs[i], None)).all()) for c in crits[i]):
                        continue
                    go_on.append(i)
                active = go_on
                if not active:
                    break
        return [SimpleNamespace(sequences=seqs[i], hidden_states=tuple(hidden[i])) for i in range(n_req)]


def get_all_objs(s):
    """reference pipeline.py:281-287"""
    matched = re.compile(r'additions:(.*)\</s\>').findall(s)
    if not matched:
        return []
    return re.compile('([^:]+):<video>').findall(matched[0])


def parse_generation(sequences, prompt_len, hidden_states, text, aux_info, mm_data, predictor, video_id, base_id, im_gen_id):
    """pipeline.py:213-279 behind the `generate` call: -> (image_embeds, base_embed, output_caption, base_img_path, extra_data), or
    (None, None, <text after 'ASSISTANT:'>, None, None) when no `<im_gen>` was produced. `text` = `batch_decode(sequences)[0]`;
    `predictor` = `vae_predictor_image`; `hidden_states[i][-1][:, -1:]` = final-normed last row of step i."""
    out_seq = sequences[:, prompt_len:]
    assert len(hidden_states) == out_seq.shape[1]
    flat = out_seq.reshape(-1).cpu()
    hits = torch.where(flat == im_gen_id)[0]
    if hits.numel() == 0:
        return None, None, text.split("ASSISTANT:")[-1], None, None
    im_gem_idx = hits[-1].item()
    all_gen_tokens = torch.where(flat == video_id)[0]
    all_gen_tokens = all_gen_tokens[all_gen_tokens > im_gem_idx]
    gen_idx = all_gen_tokens[0]
    remaining_tokens = all_gen_tokens[1:]

    def predict(i):
        return predictor(hidden_states[int(i)][-1][:, -1:]).detach().float().cpu()

    image_embeds = predict(gen_idx)
    extra_embeds = [predict(idx)[0] for idx in remaining_tokens]
    extra_embeds = torch.cat(extra_embeds) if extra_embeds else torch.zeros(0, image_embeds.shape[-1])
    if len(mm_data) == 1:
        base_idx = 0
        base_embed = aux_info[0]
    else:
        gen_idx = flat.tolist().index(base_id) + 1
        base_embed = predict(gen_idx)[0]
        base_idx = torch.einsum('ac,bc->ab', base_embed.float() / base_embed.norm() * 20, aux_info.float())[0].argmax().item()
    b = mm_data[base_idx]['fname']
    all_objs = get_all_objs(text)
    if len(all_objs) != len(extra_embeds):
        all_objs = []
    extra_idx = []
    if all_objs:
        extra_idx = torch.einsum('ac,bc->ab', extra_embeds.float() / extra_embeds.norm() * 20, aux_info.float()).argmax(1)
        extra_embeds = aux_info[extra_idx]
    output_caption = re.compile(r'\[([^\]]+)\]').findall(text)[0]
    extra_data = dict(all_objs=all_objs, extra_embeds=extra_embeds, extra_idx=extra_idx)
    return image_embeds, base_embed, output_caption, b, extra_data
