"""LoRA adapters on the MI355X: the merge kernel against fp64 (tests/lora_ref.py: exact bits on the lattice, the derived bound on real values), launch independence,
host-side refusals, `ia2p_read_tensor` as the inverse of `ia2p_load_tensor`, the adapter state of a UNet (merged forward == a FRESH UNet loaded with the merged tensors,
adapter algebra, restore, no relaunch) and the pipelines' `lora_scale`. Tiny shapes and tiny configs throughout.

The merged forward is held to the bar tests/test_unet_gpu.py holds this tiny forward to against the CPU oracle (rel-L2 < 5e-3, max|d| < 2e-2 max|ref|); the synthetic
adapter is scaled so that the oracle's own merged and base outputs differ by at least ten times that bar (asserted: an adapter that does nothing would pass everything)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, PAD = -77.0, 96


def _dev(t):
    return t.to(torch.float16).to(DEV).contiguous()


def _run(case, in_place=False, offset=0):
    """ia2p_lora_merge on a case -> (out on the host, the sentinel elements behind it are intact). offset: every tensor starts that many elements into its buffer."""
    from instructany2pix_amd.lora import lora_merge
    N, K = case["N"], case["K"]

    def shifted(t):
        buf = torch.zeros(t.numel() + offset, dtype=torch.float16, device=DEV)
        buf[offset:] = _dev(t).reshape(-1)
        return buf[offset:].view(t.shape)

    ups, downs = [shifted(u) for u in case["ups"]], [shifted(d) for d in case["downs"]]
    buf = torch.full((N * K + PAD + offset,), SENTINEL, dtype=torch.float16, device=DEV)
    out = buf[offset:offset + N * K].view(N, K)
    if in_place:
        out.copy_(_dev(case["base"]))
        base = out
    else:
        base = shifted(case["base"])
        before = base.clone()
    lora_merge(base, ups, downs, case["coefs"], out=out)
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(base, before)                                # the operands are only read
    return out.cpu(), bool((buf[offset + N * K:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


# ---- 1. the kernel against fp64 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,ranks", R.CASES)
def test_merge_lattice_gives_the_exact_bits(N, K, ranks):
    case = R.lora_case(N, K, ranks, lattice=True)
    ref, bound = R.lora_ref(case)
    assert bound is None
    out, intact = _run(case)
    R.accept(f"lora_merge lattice {N} x {K} ranks {ranks}", out, ref, None, ("row", "col"))
    assert intact


@pytest.mark.parametrize("N,K,ranks", R.CASES)
def test_merge_real_values_within_the_bound(N, K, ranks):
    case = R.lora_case(N, K, ranks, lattice=False)
    ref, bound = R.lora_ref(case)
    out, intact = _run(case)
    n = R.accept(f"lora_merge real {N} x {K} ranks {ranks}", out, ref, bound, ("row", "col"))
    print(f"lora_merge real {N} x {K} ranks {ranks}: max(err / bound) {n:.3f}")
    assert intact


def test_merge_in_place_and_through_the_guarded_path():
    case = R.lora_case(129, 264, (7, 32), lattice=False)
    ref, bound = R.lora_ref(case)
    out, intact = _run(case)
    inp, intact2 = _run(case, in_place=True)
    R.accept("lora_merge in place", inp, ref, bound, ("row", "col"))
    assert torch.equal(inp, out) and intact and intact2                 # out == base: the same bits as out of place
    # the same operands one element into their buffers: no 16-byte access is possible, every load and store is the guarded 2-byte one -> the same bits
    off, intact3 = _run(case, offset=1)
    assert torch.equal(off, out) and intact3
    lat = R.lora_case(40, 72, (4,), lattice=True)
    off, intact4 = _run(lat, offset=3)
    R.accept("lora_merge lattice, unaligned", off, R.lora_ref(lat)[0], None, ("row", "col"))
    assert intact4


def test_merge_is_independent_of_the_launch():
    """rows 5 .. 20 and columns 64 .. 135 of the 129 x 264 case, merged alone, are the bits of that slice of the full merge"""
    N, K, ranks = R.SLICE_CASE
    (r0, r1), (c0, c1) = R.SLICE_ROWS, R.SLICE_COLS
    for lattice in (False, True):
        case = R.lora_case(N, K, ranks, lattice)
        full, _ = _run(case)
        part = dict(case, N=r1 - r0, K=c1 - c0, base=case["base"][r0:r1, c0:c1].contiguous(), ups=[u[r0:r1].contiguous() for u in case["ups"]],
                    downs=[d[:, c0:c1].contiguous() for d in case["downs"]])
        alone, intact = _run(part)
        assert torch.equal(alone, full[r0:r1, c0:c1]) and intact, lattice


def test_merge_refusals_come_from_the_host():
    from instructany2pix_amd import _ffi
    lib, s, p = _ffi.lib(), _ffi.current_stream(), _ffi.ptr
    N, K, r = 16, 64, 4
    base = torch.zeros(N * K + 64, dtype=torch.float16, device=DEV)
    buf = torch.full((N * K + PAD,), SENTINEL, dtype=torch.float16, device=DEV)
    up, down = torch.zeros(N, r, dtype=torch.float16, device=DEV), torch.zeros(r, K, dtype=torch.float16, device=DEV)
    arr = lambda t, *v: (t * len(v))(*v)
    ups, downs, ranks, coefs = arr(C.c_void_p, up.data_ptr()), arr(C.c_void_p, down.data_ptr()), arr(C.c_int, r), arr(C.c_float, 1.0)
    good = dict(stream=s, base=p(base), out=p(buf), N=N, K=K, n=1, up=ups, down=downs, rank=ranks, coef=coefs)

    def call(**kw):
        a = dict(good, **kw)
        st = lib.ia2p_lora_merge(a["stream"], a["base"], a["out"], a["N"], a["K"], a["n"], a["up"], a["down"], a["rank"], a["coef"])
        if st:
            assert lib.ia2p_last_error(None), kw                          # a message through ia2p_last_error(NULL)
        return st

    for name in ("base", "out", "up", "down", "rank", "coef"):
        assert call(**{name: None}) == 1, name                            # IA2P_ERR_INVALID
    assert call(up=arr(C.c_void_p, None)) == 1 and call(down=arr(C.c_void_p, None)) == 1
    assert call(n=0) == 1 and call(n=9) == 1 and call(n=-1) == 1
    assert call(rank=arr(C.c_int, 0)) == 1 and call(rank=arr(C.c_int, 257)) == 1 and call(rank=arr(C.c_int, -4)) == 1
    assert call(coef=arr(C.c_float, float("nan"))) == 1
    assert call(N=0) == 2 and call(K=0) == 2 and call(N=-3) == 2 and call(K=-64) == 2      # IA2P_ERR_SHAPE
    assert call(base=C.c_void_p(buf.data_ptr() + 2 * K)) == 1             # out overlaps base, and is not base: base one row behind out ...
    assert call(base=p(buf), out=C.c_void_p(buf.data_ptr() + 2 * K)) == 1                  # ... and one row in front of it
    assert call(up=arr(C.c_void_p, buf.data_ptr() + 32)) == 1             # a factor inside out
    with pytest.raises(ValueError, match="INVALID"):
        _ffi.check(call(n=9))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                                  # no refused call launched anything
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((buf[:N * K] == 0).all()) and bool((buf[N * K:] == SENTINEL).all())


# ---- 2. ia2p_read_tensor --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_unet():
    from instructany2pix_amd.config import tiny
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    from instructany2pix_amd.weights import ip_adapter_specs, synthetic_state_dict, unet_param_specs
    cfg = tiny()
    sd = synthetic_state_dict(unet_param_specs(cfg), seed=7)
    ipsd = synthetic_state_dict(ip_adapter_specs(cfg, 64)["ip_adapter"], seed=7)
    hip = HipUNet2DConditionModel(cfg, DEV)
    hip.load_state_dict(sd)
    return cfg, sd, ipsd, hip


TB = "down_blocks.1.attentions.0.transformer_blocks.0"
KIND_KEYS = {"PK_COPY (a row range of the stacked QKV)": f"{TB}.attn1.to_k.weight", "PK_COPY (stacked time_emb_proj)": "up_blocks.1.resnets.2.time_emb_proj.weight",
             "PK_COPY (stacked context K/V)": f"{TB}.attn2.to_v.weight", "PK_COPY (a vector)": "conv_norm_out.bias",
             "PK_CONV": "down_blocks.1.resnets.0.conv1.weight", "PK_CONV_TAP": "conv_out.weight", "PK_GEGLU_W": f"{TB}.ff.net.0.proj.weight",
             "PK_GEGLU_B": f"{TB}.ff.net.0.proj.bias", "PK_PAD_CONV_IN": "conv_in.weight"}


@pytest.mark.parametrize("kind", list(KIND_KEYS))
def test_read_tensor_returns_the_loaded_bits(tiny_unet, kind):
    cfg, sd, ipsd, hip = tiny_unet
    key = KIND_KEYS[kind]
    want = sd[key].to(torch.float16)
    buf = torch.full((want.numel() + PAD,), SENTINEL, dtype=torch.float16, device=DEV)
    from instructany2pix_amd import _ffi
    shape = (C.c_int64 * want.ndim)(*want.shape)
    _ffi.check(hip._lib.ia2p_read_tensor(hip._ctx, key.encode(), _ffi.ptr(buf), shape, want.ndim, _ffi.current_stream()), hip._ctx)
    torch.cuda.synchronize()
    assert torch.equal(buf[:want.numel()].view(want.shape).cpu(), want.cpu()) and bool((buf[want.numel():] == SENTINEL).all())
    assert torch.equal(hip.read_tensor(key, want.shape).cpu(), want.cpu())


def test_read_tensor_refusals(tiny_unet):
    from instructany2pix_amd import _ffi
    cfg, sd, ipsd, hip = tiny_unet
    with pytest.raises(KeyError):
        hip.read_tensor("down_blocks.7.nothing.weight", (4, 4))
    with pytest.raises(ValueError, match="SHAPE"):
        hip.read_tensor("conv_in.weight", (64, 4, 3, 2))
    ipkey = next(iter(ipsd))
    with pytest.raises(_ffi.IA2PError, match="never loaded"):             # an optional key nobody loaded
        hip.read_tensor("ip_adapter." + ipkey, ipsd[ipkey].shape)
    assert hip._lib.ia2p_read_tensor(hip._ctx, b"conv_in.weight", None, (C.c_int64 * 1)(64 * 36), 1, None) == 1


# ---- 3. the adapter state of a UNet -----------------------------------------------------------------------------------------------------------------------------
LORA_MODULES = [f"{TB}.attn1.to_q", f"{TB}.attn1.to_k", f"{TB}.attn1.to_v", f"{TB}.attn1.to_out.0", f"{TB}.attn2.to_q", f"{TB}.attn2.to_k", f"{TB}.attn2.to_v",
                f"{TB}.attn2.to_out.0", "mid_block.attentions.0.transformer_blocks.1.attn2.to_k", "up_blocks.0.attentions.1.transformer_blocks.0.attn1.to_v",
                f"{TB}.ff.net.0.proj", "down_blocks.1.resnets.0.conv1", "down_blocks.1.resnets.0.conv_shortcut", "up_blocks.2.resnets.1.conv_shortcut",
                "up_blocks.1.resnets.0.time_emb_proj"]
ADAPTER_SCALE = 0.6          # factor entries ~ N(0, ADAPTER_SCALE^2 / fan): chosen on the CPU oracle so that the adapter moves the output by > 10 x the parity bar


def make_adapter(cfg, modules, rank, seed, scale=ADAPTER_SCALE, alpha=None):
    """a seeded synthetic adapter in the PEFT spelling; odd ranks and an alpha that is not the rank on purpose"""
    from instructany2pix_amd.lora import unet_lora_modules
    mods = unet_lora_modules(cfg)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, m in enumerate(modules):
        shape = mods[m]
        r = rank + (i % 3)
        K = 1
        for d in shape[1:]:
            K *= d
        sd[f"unet.{m}.lora_A.weight"] = (torch.randn((r,) + tuple(shape[1:]), generator=g) * scale * K ** -0.5).half()
        sd[f"unet.{m}.lora_B.weight"] = (torch.randn((shape[0], r) + ((1, 1) if len(shape) == 4 else ()), generator=g) * scale * r ** -0.5).half()
        sd[f"unet.{m}.alpha"] = torch.tensor(float(alpha if alpha is not None else r) * (0.75 if i % 2 else 1.0))
    return sd


def merged_state_dict(cfg, sd, adapters, weights, on_device=True):
    """the UNet's state dict with `adapters` (parsed) merged in at `weights`: on the device by ia2p_lora_merge, or in fp64 rounded to fp16 once (the oracle's weights)"""
    from instructany2pix_amd.lora import lora_coef, lora_merge
    out = dict(sd)
    for m in {m for ad in adapters for m in ad}:
        key = m + ".weight"
        use = [(ad[m], w) for ad, w in zip(adapters, weights) if m in ad and w != 0.0]
        if not use:
            continue
        coefs = [lora_coef(w, a, d.shape[0]) for (d, u, a), w in use]
        if on_device:
            out[key] = lora_merge(_dev(sd[key]), [_dev(u) for (d, u, a), w in use], [_dev(d) for (d, u, a), w in use], coefs)
        else:
            acc = sd[key].double().reshape(sd[key].shape[0], -1).half().double()
            for ((d, u, a), w), c in zip(use, coefs):
                acc = acc + c * (u.double() @ d.double())
            out[key] = R.round16(acc).reshape(sd[key].shape).float()
    if on_device:
        torch.cuda.synchronize()
    return out


def _inputs(cfg, B, h, w, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, h, w, generator=g).half()
    ctx = torch.randn(B, L, cfg.cross_attention_dim, generator=g).half()
    te = torch.randn(B, cfg.pooled_dim, generator=g).half()
    tid = torch.tensor([[h * 8.0, w * 8.0, 0, 0, h * 8.0, w * 8.0]] * B).half()
    return x, ctx, te, tid


def _install_ip(hip, cfg, ipsd, scale):
    from instructany2pix_amd.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
    from instructany2pix_amd.weights import hidden_size_of
    if ipsd is None:
        hip.set_attn_processor(AttnProcessor2_0())
        return
    procs = {}
    for n in hip.attn_processors:
        procs[n] = AttnProcessor2_0() if n.endswith("attn1.processor") else \
            IPAttnProcessor2_0(hidden_size_of(cfg, n), cfg.cross_attention_dim, scale=scale, num_tokens=4).to(DEV, torch.float16)
    hip.set_attn_processor(procs)
    torch.nn.ModuleList(hip.attn_processors.values()).load_state_dict(ipsd)


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _touched_bits(hip, modules):
    from instructany2pix_amd.lora import unet_lora_modules
    mods = unet_lora_modules(hip.config)
    return {m: hip.read_tensor(m + ".weight", mods[m]).clone() for m in modules}


@pytest.fixture()
def clean_unet(tiny_unet):
    cfg, sd, ipsd, hip = tiny_unet
    hip.unload_lora()
    _install_ip(hip, cfg, None, 0.0)
    yield tiny_unet
    hip.unload_lora()
    _install_ip(hip, cfg, None, 0.0)


@pytest.mark.parametrize("ip", [False, True], ids=["text", "ip_adapter"])
def test_merged_forward_equals_a_fresh_unet_and_meets_the_oracle_bar(clean_unet, ip):
    import oracle
    from instructany2pix_amd.lora import parse_lora_state_dict
    from instructany2pix_amd.unet import HipUNet2DConditionModel
    cfg, sd, ipsd, hip = clean_unet
    L = 81 if ip else 77
    x, ctx, te, tid = _inputs(cfg, 2, 16, 16, L, seed=11)
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=dict(text_embeds=te.to(DEV), time_ids=tid.to(DEV)))
    _install_ip(hip, cfg, ipsd if ip else None, 0.8)
    before = hip(x.to(DEV), 501, **kw)[0].clone()                        # the cached context K/V of this context tensor are warm from here on
    asd = make_adapter(cfg, LORA_MODULES, rank=5, seed=3)
    hip.load_lora_adapter(asd, "style")
    assert hip.active_adapters() == [] and torch.equal(hip(x.to(DEV), 501, **kw)[0], before)      # loaded, not active: nothing changed
    hip.set_adapters(["style"], 0.8)
    assert hip.active_adapters() == [("style", 0.8)]
    merged = hip(x.to(DEV), 501, **kw)[0].clone()                        # the SAME context tensor object: stale K/V, folds or concatenated rows would show here
    parsed = parse_lora_state_dict(asd, cfg)
    fresh = HipUNet2DConditionModel(cfg, DEV)
    fresh.load_state_dict(merged_state_dict(cfg, sd, [parsed], [0.8]))
    _install_ip(fresh, cfg, ipsd if ip else None, 0.8)
    assert torch.equal(merged, fresh(x.to(DEV), 501, **kw)[0])
    # against the CPU oracle on fp64-merged weights rounded to fp16: the bar of tests/test_unet_gpu.py for this forward
    osd = merged_state_dict(cfg, sd, [parsed], [0.8], on_device=False)
    added = dict(text_embeds=te.float(), time_ids=tid.float())
    with torch.no_grad():
        ref = (oracle.build_unet(cfg, osd, ipsd, ip_scale=0.8) if ip else oracle.build_unet(cfg, osd))(x.float(), 501, ctx.float(), added_cond_kwargs=added)[0]
        ref0 = (oracle.build_unet(cfg, sd, ipsd, ip_scale=0.8) if ip else oracle.build_unet(cfg, sd))(x.float(), 501, ctx.float(), added_cond_kwargs=added)[0]
    assert rel_l2(merged, ref) < 5e-3, rel_l2(merged, ref)
    assert float((merged.float().cpu() - ref).abs().max()) < 2e-2 * float(ref.abs().max())
    assert rel_l2(ref, ref0) > 10 * 5e-3, rel_l2(ref, ref0)             # the adapter has an effect: ten times the bar, on the oracle alone
    assert rel_l2(before, ref0) < 5e-3


def test_adapter_algebra_restore_and_no_relaunch(clean_unet, monkeypatch):
    from instructany2pix_amd import lora as Lm
    cfg, sd, ipsd, hip = clean_unet
    x, ctx, te, tid = _inputs(cfg, 1, 16, 16, 77, seed=5)
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=dict(text_embeds=te.to(DEV), time_ids=tid.to(DEV)))
    fwd = lambda: hip(x.to(DEV), 261, **kw)[0].clone()
    base_out = fwd()
    a_sd, b_sd = make_adapter(cfg, LORA_MODULES[:12], rank=4, seed=21), make_adapter(cfg, LORA_MODULES[6:], rank=9, seed=22)
    pa, pb = Lm.parse_lora_state_dict(a_sd, cfg), Lm.parse_lora_state_dict(b_sd, cfg)
    touched = sorted(set(pa) | set(pb))
    pristine = {m: _dev(sd[m + ".weight"]) for m in touched}
    assert all(torch.equal(v, pristine[m]) for m, v in _touched_bits(hip, touched).items())
    hip.load_lora_adapter(a_sd, "a")
    hip.load_lora_adapter(b_sd, "b")
    with pytest.raises(ValueError):
        hip.load_lora_adapter(a_sd, "a")                                  # the name is taken
    with pytest.raises(ValueError):
        hip.set_adapters(["a", "c"])
    with pytest.raises(ValueError):
        hip.set_adapters(["a", "b"], [1.0])

    # two adapters at (0.7, -0.4) == ONE merge with both in the list, in list order
    hip.set_adapters(["a", "b"], [0.7, -0.4])
    want = merged_state_dict(cfg, sd, [pa, pb], [0.7, -0.4])
    direct = _touched_bits(hip, touched)
    for m in touched:
        assert torch.equal(direct[m], _dev(want[m + ".weight"])), m
    out_direct = fwd()
    assert not torch.equal(out_direct, base_out)
    # ... and arriving there via (1, 1): merged again FROM THE PRISTINE COPY, never from the merged weight
    hip.set_adapters(["a", "b"], [1.0, 1.0])
    assert not torch.equal(_touched_bits(hip, touched)[touched[0]], direct[touched[0]])
    hip.set_adapters(["a", "b"], [0.7, -0.4])
    via = _touched_bits(hip, touched)
    assert all(torch.equal(via[m], direct[m]) for m in touched)
    assert torch.equal(fwd(), out_direct)

    # the same state twice launches nothing
    calls = {"merge": 0, "load": 0}
    real_merge, real_load = Lm.lora_merge, hip._load
    monkeypatch.setattr(Lm, "lora_merge", lambda *a, **k: (calls.__setitem__("merge", calls["merge"] + 1), real_merge(*a, **k))[1])
    monkeypatch.setattr(hip, "_load", lambda *a, **k: (calls.__setitem__("load", calls["load"] + 1), real_load(*a, **k))[1])
    hip.set_adapters(["a", "b"], [0.7, -0.4])
    hip.enable_lora()
    assert calls == {"merge": 0, "load": 0}
    hip.set_adapters(["a", "b"], [0.7, -0.5])                             # only b's weight moved: only the weights b touches are merged again
    assert calls["merge"] == calls["load"] == len(pb)
    hip.set_adapters(["a", "b"], [0.7, -0.4])
    monkeypatch.undo()

    # restore: disable -> the loaded bits and the forward from before any adapter; enable -> the merged bits again
    gen = hip._weights_gen
    hip.disable_lora()
    assert hip._weights_gen > gen and hip.active_adapters() == []
    off = _touched_bits(hip, touched)
    assert all(torch.equal(off[m], pristine[m]) for m in touched)
    assert torch.equal(fwd(), base_out)
    hip.enable_lora()
    on = _touched_bits(hip, touched)
    assert all(torch.equal(on[m], direct[m]) for m in touched) and torch.equal(fwd(), out_direct)
    # weight 0 and a deleted adapter contribute nothing: a alone
    hip.set_adapters(["a", "b"], [0.7, 0.0])
    only_a = _touched_bits(hip, touched)
    want_a = merged_state_dict(cfg, sd, [pa], [0.7])
    assert all(torch.equal(only_a[m], _dev(want_a[m + ".weight"])) for m in touched)
    hip.set_adapters(["a", "b"], [0.7, -0.4])
    hip.delete_adapters(["b"])
    assert hip.active_adapters() == [("a", 0.7)]
    assert all(torch.equal(v, only_a[m]) for m, v in _touched_bits(hip, touched).items())
    assert set(hip.lora.pristine) == set(pa)                              # the copies of the weights only b touched are released
    hip.unload_lora()
    assert hip.lora.pristine == {} and hip.lora.adapters == {} and hip.active_adapters() == []
    assert all(torch.equal(v, pristine[m]) for m, v in _touched_bits(hip, touched).items())
    assert torch.equal(fwd(), base_out)


# ---- 4. the pipelines ------------------------------------------------------------------------------------------------------------------------------------------
class Models:
    def __init__(self):
        from instructany2pix_amd.config import tiny, tiny_refiner
        from instructany2pix_amd.unet import HipUNet2DConditionModel
        from instructany2pix_amd.weights import ip_adapter_specs, synthetic_state_dict, unet_param_specs
        self.bcfg, self.rcfg = tiny(), tiny_refiner()
        bsd, rsd = synthetic_state_dict(unet_param_specs(self.bcfg), seed=7), synthetic_state_dict(unet_param_specs(self.rcfg), seed=11)
        specs = ip_adapter_specs(self.bcfg, 64)
        self.ck = {"image_proj": synthetic_state_dict(specs["image_proj"], seed=7), "ip_adapter": synthetic_state_dict(specs["ip_adapter"], seed=7)}
        self.base, self.ref = HipUNet2DConditionModel(self.bcfg, DEV), HipUNet2DConditionModel(self.rcfg, DEV)
        self.base.load_state_dict(bsd)
        self.ref.load_state_dict(rsd)

    def cond(self, seed, hw=16):
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)
        emb = lambda cfg: dict(prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(), pooled_prompt_embeds=rn(1, cfg.pooled_dim).half(),
                               negative_prompt_embeds=rn(1, 77, cfg.cross_attention_dim).half(), negative_pooled_prompt_embeds=rn(1, cfg.pooled_dim).half())
        c = dict(image_embeds=rn(1, 64), base_embed=rn(1, 64), y=rn(1, 64), caption=f"a photo {seed}", base_latents=rn(1, 4, hw, hw).half(), **emb(self.bcfg),
                 polar_noise=rn(1, 4, hw, hw).half(), refiner_noise=rn(1, 4, hw, hw).half(), subject_data=[])
        c.update({"refiner_" + k: v for k, v in emb(self.rcfg).items()})
        return c

    def pipeline(self, conds):
        from instructany2pix_amd.pipeline import InstructAny2PixPipeline
        pipe = InstructAny2PixPipeline(unet=self.base, ip_ckpt=self.ck, device=DEV, clip_embeddings_dim=64, conditioner=lambda inst, mm, use_cache=False: conds[inst],
                                       refiner_unet=self.ref, refiner_handoff="latent")
        pipe.ip_adapter_xl.set_scale(1.0)
        return pipe


REFINER_MODULES = ["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q", "mid_block.attentions.0.transformer_blocks.1.attn2.to_v", "up_blocks.1.resnets.0.conv_shortcut"]


def test_pipeline_lora_scale_is_set_adapters_for_one_call():
    m = Models()
    conds = {"one": m.cond(61), "two": m.cond(62)}
    pipe = m.pipeline(conds)
    call = lambda **kw: pipe("one", [], num_inference_steps=3, refinement=0.1, seed=9, **kw)
    plain = call()
    assert torch.equal(call(lora_scale=None)[1], plain[1]) and torch.equal(call(lora_scale=0.5)[1], plain[1])      # no adapter: nothing to scale, the same bits
    pipe.load_lora_weights(make_adapter(m.bcfg, LORA_MODULES, rank=4, seed=31), "style", text_encoder_keys="skip")
    pipe.load_lora_weights(make_adapter(m.rcfg, REFINER_MODULES, rank=6, seed=32), "finish", target="refiner")
    assert pipe.get_active_adapters() == ["style"] and pipe.get_active_adapters("refiner") == ["finish"]           # active at weight 1, as diffusers does
    with pytest.raises(ValueError):
        pipe.load_lora_weights({}, "x", target="decoder")
    pipe.set_adapters(["style"], [0.8])
    full = call()
    assert not torch.equal(full[0], plain[0]) and not torch.equal(full[1], full[0])
    state = (m.base.active_adapters(), m.ref.active_adapters())
    bits = _touched_bits(m.base, LORA_MODULES[:3])
    scaled = call(lora_scale=0.5)
    assert (m.base.active_adapters(), m.ref.active_adapters()) == state == ([("style", 0.8)], [("finish", 1.0)])    # the state before is back
    assert all(torch.equal(v, bits[k]) for k, v in _touched_bits(m.base, LORA_MODULES[:3]).items())
    pipe.set_adapters(["style"], [0.8 * 0.5])
    pipe.set_adapters(["finish"], [0.5], target="refiner")
    by_hand = call()
    assert torch.equal(scaled[0], by_hand[0]) and torch.equal(scaled[1], by_hand[1])
    assert not torch.equal(scaled[0], full[0]) and not torch.equal(scaled[1], full[1])
    # the state comes back when the call raises, too
    pipe.set_adapters(["style"], [0.8])
    pipe.set_adapters(["finish"], [1.0], target="refiner")
    with pytest.raises(KeyError):
        pipe("no such request", [], num_inference_steps=3, lora_scale=0.25)
    assert (m.base.active_adapters(), m.ref.active_adapters()) == state
    assert all(torch.equal(v, bits[k]) for k, v in _touched_bits(m.base, LORA_MODULES[:3]).items())
    assert torch.equal(call()[1], full[1])

    # edit_batch: one scale for the whole call
    batch = lambda **kw: pipe.edit_batch(["one", "two"], [[], []], num_inference_steps=3, refinement=0.1, seeds=[9, 10], group=2, **kw)
    b_full = batch()
    b_scaled = batch(lora_scale=0.5)
    assert (m.base.active_adapters(), m.ref.active_adapters()) == state
    pipe.set_adapters(["style"], [0.4])
    pipe.set_adapters(["finish"], [0.5], target="refiner")
    b_hand = batch()
    for i in range(2):
        assert torch.equal(b_scaled[i][0], b_hand[i][0]) and torch.equal(b_scaled[i][1], b_hand[i][1]), i
        assert not torch.equal(b_scaled[i][1], b_full[i][1]), i
    with pytest.raises(ValueError):
        pipe.edit_batch(["one"], [[], []], lora_scale=0.5)
    assert m.base.active_adapters() == [("style", 0.4)]
    # disable / unload on the pipeline reach both UNets: the bits of the pipeline without adapters
    pipe.disable_lora()
    assert torch.equal(call()[1], plain[1])
    pipe.enable_lora()
    assert torch.equal(call()[1], by_hand[1])
    pipe.unload_lora_weights()
    assert pipe.get_active_adapters() == [] and torch.equal(call()[1], plain[1])
