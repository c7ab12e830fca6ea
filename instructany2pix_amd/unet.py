"""HIP-backed conditional UNet with the call surface the reference uses on diffusers' UNet2DConditionModel.

What callers in the reference touch, and where it lives here:
  unet(sample, t, encoder_hidden_states=, cross_attention_kwargs=None, added_cond_kwargs={...}, return_dict=False)[0]
        instructany2pix/ddim/pnp_pipeline.py:253-260; ddim/sdxl_pipeline.py:832-839          -> __call__
  unet.config.{in_channels, addition_time_embed_dim, cross_attention_dim, block_out_channels, sample_size}
        pnp_pipeline.py:44-47; diffusion/ip_adapter/ip_adapter.py:114,124-132                   -> .config
  unet.add_embedding.linear_1.in_features       pnp_pipeline.py:47                            -> .add_embedding
  unet.attn_processors / unet.set_attn_processor(...)   ip_adapter.py:123,142,154,168          -> same names
All arithmetic runs in libia2p_hip.so (`ia2p_unet_forward_x`); this class owns the flat weight arena and the
activation workspace as torch tensors (device memory plumbing only) and keeps no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, Iterable, Optional, Tuple, Union

import torch

from . import _ffi
from .attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
from .config import UNetConfig
from .weights import attn_processor_names


_CALL_SIZE = C.sizeof(_ffi.UNetCallC)


def per_row(value, B: int, name: str, device, broadcast: bool = True) -> torch.Tensor:
    """`value` -- a number, a one-element tensor (both stand for every row, unless `broadcast` is off) or B values -- as a contiguous float32 [B] device tensor"""
    t = torch.full((B,), float(value)) if isinstance(value, (int, float)) else torch.as_tensor(value)
    t = t.to(device=device, dtype=torch.float32).reshape(-1)
    if broadcast and t.numel() == 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"{name} has {t.numel()} elements for a batch of {B}")
    return t.contiguous()


def _inputs(model, sample, encoder_hidden_states, added_cond_kwargs):
    """What every forward of the UNet's kind (this UNet, `HipControlNetModel`) takes, checked against `model.config` and as contiguous fp16 tensors on `model.device`:
    -> sample, context, text_embeds, time_ids, (B, h, w, L)"""
    cfg = model.config
    if encoder_hidden_states is None or added_cond_kwargs is None:
        raise ValueError("encoder_hidden_states and added_cond_kwargs (text_embeds, time_ids) are required (text_time UNet)")
    if "text_embeds" not in added_cond_kwargs or "time_ids" not in added_cond_kwargs:
        raise ValueError("added_cond_kwargs must carry `text_embeds` and `time_ids`")      # diffusers raises ValueError here too
    B, c_in, h, w = sample.shape
    if c_in != cfg.in_channels:
        raise ValueError(f"sample has {c_in} channels, expected {cfg.in_channels}")
    f16 = lambda t: t.to(device=model.device, dtype=torch.float16).contiguous()      # noqa: E731
    sample, ctx = f16(sample), f16(encoder_hidden_states)
    te, tid = f16(added_cond_kwargs["text_embeds"]), f16(added_cond_kwargs["time_ids"])
    if ctx.shape[0] != B or ctx.shape[2] != cfg.cross_attention_dim:
        raise ValueError(f"encoder_hidden_states must be [B, L, {cfg.cross_attention_dim}]")
    if te.shape != (B, cfg.pooled_dim) or tid.shape != (B, cfg.num_time_ids):
        raise ValueError(f"Model expects an added time embedding vector of length {cfg.projection_class_embeddings_input_dim}, "
                         f"but a vector of {te.shape[-1] + tid.shape[-1] * cfg.addition_time_embed_dim} was created.")
    return sample, ctx, te, tid, (B, h, w, ctx.shape[1])


class HipUNet2DConditionModel(_ffi.Executor):
    dtype = torch.float16
    _lora = None                        # lora.LoraManager, created when the first adapter is loaded (class default: a stand-in that skipped the constructor has none)

    def __init__(self, config: UNetConfig, device: Union[str, torch.device] = "cuda:0"):
        config.validate()
        self.config = config
        super().__init__("", _ffi.make_config(config), device)
        torch.cuda.set_device(self.device)       # process-wide and left set: callers rely on it (the forward takes no device guard of its own)
        self._ctx = self._h                      # (the name the forward, bench.py and the tools use for the handle)
        self._ws_key = None
        # context K/V hoisting: the cross-attention K/V projections of a context are computed once and reused while the SAME context
        # tensor object (unmodified: torch's version counter) keeps arriving, i.e. over the denoise steps of a request
        self.cache_context_kv = True
        self._kv = None                 # (context tensor kept alive, its _version, ip (enabled, tokens), weight generation, kv buffer)
        self._weights_gen = 0
        self._names = attn_processor_names(config)
        self._procs: "OrderedDict[str, torch.nn.Module]" = OrderedDict((n, AttnProcessor2_0()) for n in self._names)
        self._ip_sig = None
        self.add_embedding = SimpleNamespace(linear_1=SimpleNamespace(in_features=config.projection_class_embeddings_input_dim))

    # ---- weights --------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Union[Dict[str, torch.Tensor], Iterable[Tuple[str, torch.Tensor]]], strict: bool = True):
        """Load parameters by diffusers key. Accepts a dict or an iterator of (key, tensor) so 5 GB of weights
        never need to be resident twice."""
        items = state_dict.items() if hasattr(state_dict, "items") else state_dict
        torch.cuda.set_device(self.device)
        for k, v in items:
            self._load(k, v)
        torch.cuda.synchronize(self.device)
        if strict:
            self.finalize()

    def _load(self, key: str, v: torch.Tensor):
        self._weights_gen += 1
        self.load_tensor(key, v)

    def read_tensor(self, key: str, shape) -> torch.Tensor:
        """The parameter `key` as it was loaded: fp16, the checkpoint's layout and bits (`ia2p_read_tensor`, the inverse of `load_tensor`)."""
        shape = tuple(int(d) for d in shape)
        t = torch.empty(shape, dtype=torch.float16, device=self.device)
        with self._on_device():
            self.check(self._lib.ia2p_read_tensor(self._ctx, key.encode(), _ffi.ptr(t), (C.c_int64 * len(shape))(*shape), len(shape), _ffi.current_stream()))
        return t

    @property
    def arena_raw(self) -> torch.Tensor:
        """Head of the arena: the parameters as loaded (5.8 GB for SDXL-base + IP-Adapter). The tail behind it holds data derived at
        finalize (LayerNorm-folded weight copies, 2.5 GB) that every rank can recompute: only this view needs to travel."""
        return self.arena[: self._lib.ia2p_arena_raw_bytes(self._ctx)]

    def adopt_arena(self, with_ip_adapter: bool = True):
        """The arena HEAD was produced elsewhere (RCCL broadcast of `arena_raw` from rank 0): mark parameters present and derive the
        tail (LayerNorm folds) locally with the same kernel rank 0 used, so ranks hold bit-identical arenas."""
        _ffi.check(self._lib.ia2p_adopt_arena_on(self._ctx, int(with_ip_adapter), _ffi.current_stream()), self._ctx)   # ordered behind the broadcast
        self._weights_gen += 1

    # ---- LoRA adapters (lora.py) --------------------------------------------------------------------------
    @property
    def lora(self):
        """The adapter state of this UNet (`lora.LoraManager`), created at first use."""
        if self._lora is None:
            from .lora import LoraManager
            self._lora = LoraManager(self)
        return self._lora

    def load_lora_adapter(self, path_or_dict, adapter_name: str = "default", **parse_kw):
        """Read an adapter (`.safetensors` path or state dict, `lora.parse_lora_state_dict`) onto the device under `adapter_name`. It is not active
        until `set_adapters` names it."""
        self.lora.load(path_or_dict, adapter_name, **parse_kw)

    def set_adapters(self, names, weights=1.0):
        """The active adapters and their weights (one number for all, or one per name): every touched weight whose contribution changes is merged again
        from its pristine copy (`ia2p_lora_merge`) and reloaded; the same state twice launches nothing."""
        self.lora.set_adapters(names, weights)

    def disable_lora(self):
        """The weights as loaded, bit for bit; the adapters and the active set are kept for `enable_lora`."""
        if self._lora is not None:
            self._lora.disable()

    def enable_lora(self):
        if self._lora is not None:
            self._lora.enable()

    def delete_adapters(self, names):
        self.lora.delete(names)

    def unload_lora(self):
        """The weights as loaded, and every adapter and pristine copy released."""
        if self._lora is not None:
            self._lora.unload()

    def active_adapters(self):
        """[(adapter name, weight)] merged into the weights now (empty while disabled)."""
        return self._lora.active_adapters() if self._lora is not None else []

    # ---- operator-plugin API (reference ip_adapter.py:120-154) ----------------------------------------------------
    @property
    def attn_processors(self) -> "OrderedDict[str, torch.nn.Module]":
        return OrderedDict(self._procs)

    def set_attn_processor(self, processor):
        if isinstance(processor, dict):
            if set(processor) != set(self._names):
                raise ValueError(f"A dict of processors was passed, but the number of processors {len(processor)} does not match "
                                 f"the number of attention layers: {len(self._names)}.")
            self._procs = OrderedDict((n, processor[n]) for n in self._names)
        else:
            self._procs = OrderedDict((n, processor) for n in self._names)
        self._ip_sig = None

    def _sync_processors(self):
        """Push the installed plugins into the HIP context when they changed (weights, scale or topology)."""
        ips = [(n, p) for n, p in self._procs.items() if isinstance(p, IPAttnProcessor2_0)]
        if not ips:
            sig = ("off",)
            if sig != self._ip_sig:
                _ffi.check(self._lib.ia2p_set_ip_adapter(self._ctx, 0, 4, 1.0), self._ctx)
                self._ip_sig = sig
            return
        bad = [n for n, p in ips if n.endswith("attn1.processor")]
        if bad or len(ips) != len(self._names) // 2:
            raise NotImplementedError("IP processors must sit on every attn2 and only there (reference ip_adapter.py:123-141)")
        scales = {float(p.scale) for _, p in ips}
        toks = {int(p.num_tokens) for _, p in ips}
        if len(scales) != 1 or len(toks) != 1:
            raise NotImplementedError("per-layer IP scales / token counts are not supported (the reference sets one value, ip_adapter.py:211-214)")
        if all(p.to_k_ip.weight.is_meta for _, p in ips):
            wsig = "arena"           # descriptors only: weights were streamed straight into the arena (load_ip_adapter_weights)
        else:
            wsig = hash(tuple((p.to_k_ip.weight.data_ptr(), p.to_k_ip.weight._version, p.to_v_ip.weight.data_ptr(), p.to_v_ip.weight._version) for _, p in ips))
        sig = ("on", scales.pop(), toks.pop(), wsig)
        if sig == self._ip_sig:
            return
        if wsig != "arena" and (self._ip_sig is None or self._ip_sig[0] != "on" or self._ip_sig[3] != sig[3]):
            for n, p in ips:
                idx = self._names.index(n)
                self._load(f"ip_adapter.{idx}.to_k_ip.weight", p.to_k_ip.weight)
                self._load(f"ip_adapter.{idx}.to_v_ip.weight", p.to_v_ip.weight)
        _ffi.check(self._lib.ia2p_set_ip_adapter(self._ctx, 1, sig[2], sig[1]), self._ctx)
        self._ip_sig = sig

    def load_ip_adapter_weights(self, items, scale: float = 1.0, num_tokens: int = 4):
        """Stream `{"<idx>.to_k_ip.weight": tensor, ...}` (the "ip_adapter" group of the checkpoint, reference
        ip_adapter.py:165-169) straight into the arena and install storage-free IP processor descriptors: the
        0.68 GB of adapter weights then exist once, in the arena, not twice."""
        from .weights import hidden_size_of
        it = items.items() if hasattr(items, "items") else items
        for k, v in it:
            self._load("ip_adapter." + k, v)
        procs = {}
        for n in self._names:
            if n.endswith("attn1.processor"):
                procs[n] = AttnProcessor2_0()
            else:
                with torch.device("meta"):
                    procs[n] = IPAttnProcessor2_0(hidden_size_of(self.config, n), self.config.cross_attention_dim, scale=scale, num_tokens=num_tokens)
        self.set_attn_processor(procs)

    # ---- forward -----------------------------------------------------------------------------------------------------
    def workspace_for(self, B: int, h: int, w: int, L: int, G: int = 0) -> torch.Tensor:
        """the workspace of a forward (`ia2p_workspace_bytes_x`); G > 0: a regional one, the plain pass's plus the mask pyramid"""
        # (ip on/off, scale, tokens); the kernel plan table decides the K-split slabs, so its generation is part of the key
        key = (B, h, w, L, self._ip_sig[:3] if self._ip_sig else None, self._lib.ia2p_plan_generation(), G)
        if self._ws_key != key:
            self.workspace(self._lib.ia2p_workspace_bytes_x(self._ctx, _ffi.UNetCallC(struct_size=_CALL_SIZE, B=B, h=h, w=w, L=L, G=G)))
            self._ws_key = key
        return self._ws

    def _channels_last(self, t, B, C_, H, W, what):
        """a logical-NCHW residual [B, C, H, W] as a channels-last device buffer: by pointer when its strides already are, converted otherwise"""
        t = torch.as_tensor(t)
        if tuple(t.shape) != (B, C_, H, W):
            raise ValueError(f"{what} has shape {tuple(t.shape)}, this UNet's tensor there is {(B, C_, H, W)}")
        t = t.to(device=self.device, dtype=torch.float16)
        nhwc = t.permute(0, 2, 3, 1)
        if not nhwc.is_contiguous() or nhwc.data_ptr() % 16:
            nhwc = nhwc.contiguous()
            if nhwc.data_ptr() % 16:
                nhwc = nhwc.clone()
        return nhwc

    def skip_shapes(self, h: int, w: int):
        """[(channels, height, width)] of the tensors the down path leaves for the up path at an h x w latent, in skip order -- the shapes of
        `down_block_additional_residuals`; the mid block's output is (block_out_channels[-1], height, width of the last entry)"""
        ch = list(self.config.block_out_channels)
        out = [(ch[0], h, w)]
        for i in range(len(ch)):
            out += [(ch[i], h, w)] * self.config.layers_per_block
            if i != len(ch) - 1:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                out.append((ch[i], h, w))
        return out

    def _region_masks(self, masks, B, h, w, L):
        """`ip_adapter_masks` as a contiguous fp16 device tensor [B, G, h, w]"""
        if self._ip_sig is None or self._ip_sig[0] != "on":
            raise ValueError("ip_adapter_masks needs the IP-Adapter processors installed (set_attn_processor / load_ip_adapter_weights)")
        m = torch.as_tensor(masks)
        if m.ndim == 3:
            m = m.unsqueeze(0).expand(B, *m.shape)
        if m.ndim != 4 or m.shape[0] != B or tuple(m.shape[2:]) != (h, w) or not 1 <= m.shape[1] <= 16:
            raise ValueError(f"ip_adapter_masks must be [B, G, h, w] or [G, h, w] on the latent grid {h} x {w} of `sample`, 1 <= G <= 16; got {tuple(m.shape)}")
        if L <= 4 * m.shape[1]:
            raise ValueError(f"encoder_hidden_states holds {L} rows: {m.shape[1]} regions need {4 * m.shape[1]} image-token rows behind the text rows")
        return m.to(device=self.device, dtype=torch.float16).contiguous()

    def _residuals(self, down, mid, B, h, w):
        """a ControlNet's residuals as channels-last device buffers, the mid residual last"""
        shapes = self.skip_shapes(h, w)
        if len(down) != len(shapes):
            raise ValueError(f"{len(down)} down_block_additional_residuals, this UNet has {len(shapes)} skips")
        keep = [self._channels_last(t, B, c_, hh, ww, f"down_block_additional_residuals[{k}]") for k, (t, (c_, hh, ww)) in enumerate(zip(down, shapes))]
        return keep + [self._channels_last(mid, B, self.config.block_out_channels[-1], shapes[-1][1], shapes[-1][2], "mid_block_additional_residual")]

    def __call__(self, sample, timestep, encoder_hidden_states=None, cross_attention_kwargs=None, added_cond_kwargs=None,
                 return_dict: bool = False, out: Optional[torch.Tensor] = None, _tune_reps: Optional[int] = None,
                 ip_scales: Optional[torch.Tensor] = None, down_block_additional_residuals=None, mid_block_additional_residual=None, **unused):
        """One evaluation: the options are resolved, the inputs marshalled once (`_inputs`), and one record goes to `ia2p_unet_forward_x` (include/ia2p.h states which
        options may meet). Every refusal comes before any launch.
        down_block_additional_residuals / mid_block_additional_residual (diffusers' names): a ControlNet's residuals, one logical-NCHW tensor per skip and one for the
        mid block's output; tensors with channels-last strides (what `HipControlNetModel` returns) are passed by pointer, others are converted. Both None: none.
        cross_attention_kwargs={"ip_adapter_masks": t} (t [B, G, h, w] on the latent grid of `sample`, or [G, h, w] for every row): regional image prompts -- the
        last 4 G rows of the context are G groups of four image tokens, group g acts where t[:, g] says (diffusers' `ip_adapter_masks`). The installed adapter's token
        count becomes 4 G for this call and is put back afterwards; context K/V cached under the other count are not reused (`_context_kv` keys them by it).
        `timestep`: a number / 0-dim tensor as the reference passes it (it travels by value), or a [B] tensor -- one timestep per batch element, as diffusers' UNet
        accepts; `ip_scales` (or cross_attention_kwargs={"ip_scales": ...}): optional [B] tensor, the IP-Adapter scale of every batch element (the reference sets one
        value per call, ip_adapter.py:211-214). Both let independent requests share one evaluation."""
        # 1. the options
        kw = cross_attention_kwargs or {}
        masks, down, mid = kw.get("ip_adapter_masks"), down_block_additional_residuals, mid_block_additional_residual
        if ip_scales is None:
            ip_scales = kw.get("ip_scales")
        if (down is None) != (mid is None):
            raise ValueError("down_block_additional_residuals and mid_block_additional_residual come together")
        if down is not None and masks is not None:
            raise ValueError("ControlNet residuals together with ip_adapter_masks: the regional pass is not combined with a ControlNet")
        per_row_call = down is not None or masks is not None or ip_scales is not None or (torch.is_tensor(timestep) and timestep.numel() > 1)
        if _tune_reps is not None and per_row_call:
            raise ValueError("autotune takes a scalar timestep and no ip_scales, ip_adapter_masks or ControlNet residuals")
        # 2. the inputs
        self._sync_processors()
        ctx_in = encoder_hidden_states
        sample, ctx, te, tid, (B, h, w, L) = _inputs(self, sample, encoder_hidden_states, added_cond_kwargs)
        m = self._region_masks(masks, B, h, w, L) if masks is not None else None
        G = int(m.shape[1]) if m is not None else 0
        res = self._residuals(list(down), mid, B, h, w) if down is not None else None
        # (a scalar timestep with no per-row option travels by value: no [B] tensor, no copy to the device)
        ts = per_row(timestep, B, "timestep tensor", self.device) if per_row_call else None
        sc = per_row(ip_scales, B, "ip_scales", self.device, broadcast=False) if ip_scales is not None else None
        if out is None:
            out = torch.empty(B, self.config.out_channels, h, w, dtype=torch.float16, device=self.device)
        call = _ffi.UNetCallC(struct_size=_CALL_SIZE, B=B, h=h, w=w, L=L, G=G, sample=_ffi.addr(sample), text_embeds=_ffi.addr(te), time_ids=_ffi.addr(tid),
                              out=_ffi.addr(out), timesteps=_ffi.addr(ts), ip_scales=_ffi.addr(sc), region_masks=_ffi.addr(m))
        if ts is None:
            call.timestep = float(timestep.item()) if torch.is_tensor(timestep) else float(timestep)
        if res is not None:
            call.n_down, call.mid_residual = len(res) - 1, _ffi.addr(res[-1])
            call.down_residuals = (C.c_void_p * call.n_down)(*[t.data_ptr() for t in res[:-1]])
        sig = self._ip_sig
        try:
            if G and sig[2] != 4 * G:
                _ffi.check(self._lib.ia2p_set_ip_adapter(self._ctx, 1, 4 * G, sig[1]), self._ctx)
                self._ip_sig = sig[:2] + (4 * G,) + sig[3:]
            # 3. the workspace, 4. the context or its cached projections, 5. + 6. the record and the call
            ws = self.workspace_for(B, h, w, L, G)
            if _tune_reps is not None:      # (ia2p_autotune keeps the scalar argument list)
                sites = C.c_int(0)
                _ffi.check(self._lib.ia2p_autotune(self._ctx, _ffi.current_stream(), _ffi.ptr(sample), call.timestep, _ffi.ptr(ctx), L, _ffi.ptr(te), _ffi.ptr(tid),
                                                   _ffi.ptr(out), B, h, w, _ffi.ptr(ws), ws.numel(), int(_tune_reps), C.addressof(sites)), self._ctx)
                return sites.value
            if self.cache_context_kv:
                ip = sig and self._ip_sig[:1] + self._ip_sig[2:3]          # (on/off, tokens): the split of the context rows
                call.kv = _ffi.addr(self._context_kv(ip, self._lib.ia2p_context_kv_bytes, self._lib.ia2p_project_context, ctx_in, ctx, B, L, ws))
            else:
                call.context = _ffi.addr(ctx)
            _ffi.check(self._lib.ia2p_unet_forward_x(self._ctx, _ffi.current_stream(), call, _ffi.ptr(ws), ws.numel()), self._ctx)
        finally:
            if self._ip_sig is not sig:
                self._ip_sig = sig
                _ffi.check(self._lib.ia2p_set_ip_adapter(self._ctx, 1, sig[2], sig[1]), self._ctx)
        return (out,) if not return_dict else SimpleNamespace(sample=out)

    def set_gn_fuse(self, mode: int):
        """GroupNorm + SiLU of the ResnetBlock2Ds: 1 (default) inside the halo-staged 3x3 convolutions that consume them (statistics from the producers' epilogues),
        0 as GroupNorm launches of their own, 2 the fused path's unfused twin (same statistics, same bits as 1; tests). `ia2p_set_gn_fuse`."""
        _ffi.check(self._lib.ia2p_set_gn_fuse(self._ctx, int(mode)), self._ctx)

    def invalidate_context_kv(self):
        """Forget the cached context K/V projections (a new request begins: the next evaluation projects its context again); the buffer is kept."""
        if self._kv is not None:
            self._kv = (None, -1, None, -1, self._kv[4], self._kv[5])

    def autotune(self, sample, timestep, encoder_hidden_states, added_cond_kwargs, reps: int = 7) -> int:
        """Measure the candidate (tile, K-split) plans of every GEMM / conv shape of this call in place and keep the fastest
        (ia2p_autotune; process-wide table, see export_plans / import_plans). Returns the number of shapes measured.
        Use inputs shaped like the real ones (random values, not zeros). Optional: without it the built-in cost model picks."""
        for _ in range(4):          # bring the clocks up first: candidates measured on a cold GPU would all look slow, the first ones most
            self(sample, timestep, encoder_hidden_states=encoder_hidden_states, added_cond_kwargs=added_cond_kwargs)
        return self(sample, timestep, encoder_hidden_states=encoder_hidden_states, added_cond_kwargs=added_cond_kwargs, _tune_reps=reps)

    # ---- per-kernel-class timing for the roofline leg of bench.py ------------------------------------------------
    def profile(self, on: bool):
        _ffi.check(self._lib.ia2p_profile_enable(self._ctx, int(on)), self._ctx)

    def profile_read_regions(self):
        """{"other" | "conv_blocks" | "transformer": dict(launches, ms, flops, bytes)} summed since profile(True): which part of the network
        the launches belonged to (conv blocks = conv_in/out, ResnetBlock2D incl. GroupNorm+SiLU and shortcuts, resample convs, concat)."""
        res = {}
        for r, name in enumerate(("other", "conv_blocks", "transformer")):
            n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            _ffi.check(self._lib.ia2p_profile_read_region(self._ctx, r, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), self._ctx)
            res[name] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)
        return res

    def profile_read_roles(self):
        """{layer role: dict(launches, ms, flops, bytes)} summed since profile(True): keyed by the executor's call site (FF-in, FF-out, QKV + self-attention,
        out-projections, to_q + cross-attention, 3x3 convolutions, GroupNorm, ...), whatever kernel instantiation the plan table picked."""
        res = {}
        for r in range(self._lib.ia2p_profile_roles()):
            name = C.create_string_buffer(128)
            n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            _ffi.check(self._lib.ia2p_profile_read_role(self._ctx, r, name, 128, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), self._ctx)
            if n.value:
                kernels = {}
                for k in range(self._lib.ia2p_profile_classes()):
                    kn, kms = C.c_int64(), C.c_double()
                    _ffi.check(self._lib.ia2p_profile_read_role_class(self._ctx, r, k, C.byref(kn), C.byref(kms)), self._ctx)
                    if kn.value:
                        kname = C.create_string_buffer(96)
                        _ffi.check(self._lib.ia2p_profile_read(self._ctx, k, kname, 96, None, None, None, None), self._ctx)
                        kernels[kname.value.decode()] = dict(launches=kn.value, ms=kms.value)
                res[name.value.decode()] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value, kernels=kernels)
        return res

    def profile_read(self):
        """{kernel name: dict(launches, ms, flops, bytes)} summed since profile(True)."""
        res = {}
        for k in range(self._lib.ia2p_profile_classes()):
            name = C.create_string_buffer(96)
            n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            _ffi.check(self._lib.ia2p_profile_read(self._ctx, k, name, 96, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), self._ctx)
            if n.value:
                pf = C.c_double()
                _ffi.check(self._lib.ia2p_profile_read_prefetch(self._ctx, k, C.byref(pf)), self._ctx)
                res[name.value.decode()] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value, prefetch_bytes=pf.value)
        return res


def export_plans() -> str:
    """measured kernel plans as text ("M,N,K,conv,geglu,variant,splitk;..."), e.g. to broadcast from rank 0"""
    lib = _ffi.lib()
    n = lib.ia2p_plan_export(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.ia2p_plan_export(buf, n + 1)
    return buf.value.decode()


def import_plans(text: str) -> int:
    n = _ffi.lib().ia2p_plan_import(text.encode())
    if n < 0:
        raise ValueError("malformed kernel plan table")
    return n


def clear_plans() -> None:
    _ffi.lib().ia2p_plan_clear()


def build_unet(config: UNetConfig, state_dict=None, device="cuda:0") -> HipUNet2DConditionModel:
    m = HipUNet2DConditionModel(config, device)
    if state_dict is not None:
        m.load_state_dict(state_dict)
    return m
