"""The five argument-list forms of the UNet callable (`ia2p_unet_forward`, `_kv`, `_v`, `_r`, `_c`) are thin callers of the record form (`ia2p_unet_forward_x`,
include/ia2p.h): each, called by ctypes, writes the output bytes of the record that says the same. config.tiny() with the synthetic IP-Adapter (4 image tokens),
B = 2, 16 x 16, L = 81; the Python classes only build the context and push the adapter state."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, L, T = 2, 16, 81, 981.0


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half().to(DEV)


class Case:
    def __init__(self):
        from instructany2pix_amd import _ffi
        from instructany2pix_amd.config import tiny
        from instructany2pix_amd.unet import HipUNet2DConditionModel
        from instructany2pix_amd.weights import ip_adapter_specs, synthetic_state_dict, unet_param_specs
        cfg = tiny()
        self.ffi, self.lib = _ffi, _ffi.lib()
        self.net = net = HipUNet2DConditionModel(cfg, DEV)
        net.load_state_dict(synthetic_state_dict(unet_param_specs(cfg), seed=7))
        net.load_ip_adapter_weights(synthetic_state_dict(ip_adapter_specs(cfg, 64)["ip_adapter"], seed=7), scale=1.0, num_tokens=4)
        self.sample, self.ctx = rnd(B, 4, H, H, seed=1), rnd(B, L, cfg.cross_attention_dim, seed=2)
        self.te, self.tid = rnd(B, cfg.pooled_dim, seed=3), torch.tensor([[128.0, 128.0, 0, 0, 128.0, 128.0]] * B).half().to(DEV)
        net(self.sample, T, encoder_hidden_states=self.ctx, added_cond_kwargs=dict(text_embeds=self.te, time_ids=self.tid))      # (pushes the adapter state into the context)
        lib, h = self.lib, net._ctx
        n = max(lib.ia2p_workspace_bytes(h, B, H, H, L), lib.ia2p_workspace_bytes_r(h, B, H, H, L, 1))
        assert n > 0
        self.ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        nkv = lib.ia2p_context_kv_bytes(h, B, L)
        self.kv = torch.empty(nkv, dtype=torch.uint8, device=DEV)
        p = _ffi.ptr
        assert lib.ia2p_project_context(h, _ffi.current_stream(), p(self.ctx), L, B, p(self.kv), nkv, p(self.ws), n) == 0
        self.ts, self.sc = torch.tensor([981.0, 441.0], device=DEV), torch.tensor([1.0, 0.4], device=DEV)
        self.masks = torch.rand(B, 1, H, H, generator=torch.Generator().manual_seed(5)).half().to(DEV)
        shapes = net.skip_shapes(H, H)
        self.res = [0.25 * rnd(B, hh, ww, c, seed=40 + k) for k, (c, hh, ww) in enumerate(shapes + [shapes[-1]])]      # channels-last buffers
        self.down = (C.c_void_p * len(shapes))(*[t.data_ptr() for t in self.res[:-1]])

    def record(self, out, **fields):
        f = self.ffi
        return f.UNetCallC(struct_size=C.sizeof(f.UNetCallC), B=B, h=H, w=H, L=L, sample=f.addr(self.sample), text_embeds=f.addr(self.te), time_ids=f.addr(self.tid),
                           out=f.addr(out), **fields)

    def forms(self, out):
        """name -> (the legacy call, the record that says the same), both writing `out`"""
        f, lib, h, p = self.ffi, self.lib, self.net._ctx, self.ffi.ptr
        head = (h, f.current_stream(), p(self.sample))
        tail = (L, p(self.te), p(self.tid), p(out), B, H, H, p(self.ws), self.ws.numel())
        a = f.addr
        per_row = dict(timesteps=a(self.ts), ip_scales=a(self.sc))
        return {
            "forward": (lambda: lib.ia2p_unet_forward(*head, T, p(self.ctx), *tail), self.record(out, timestep=T, context=a(self.ctx))),
            "kv": (lambda: lib.ia2p_unet_forward_kv(*head, T, p(self.kv), *tail), self.record(out, timestep=T, kv=a(self.kv))),
            "v": (lambda: lib.ia2p_unet_forward_v(*head, p(self.ts), p(self.sc), p(self.ctx), None, *tail), self.record(out, context=a(self.ctx), **per_row)),
            "r": (lambda: lib.ia2p_unet_forward_r(*head, p(self.ts), p(self.sc), None, p(self.kv), *tail, p(self.masks), 1),
                  self.record(out, kv=a(self.kv), region_masks=a(self.masks), G=1, **per_row)),
            "c": (lambda: lib.ia2p_unet_forward_c(*head, p(self.ts), p(self.sc), p(self.ctx), None, *tail, self.down, len(self.down), p(self.res[-1]), None, 0),
                  self.record(out, context=a(self.ctx), down_residuals=self.down, n_down=len(self.down), mid_residual=a(self.res[-1]), **per_row)),
        }


@pytest.fixture(scope="module")
def case():
    return Case()


def test_each_legacy_export_writes_the_bytes_of_its_record(case):
    out = torch.empty(B, 4, H, H, dtype=torch.half, device=DEV)
    got = {}
    for name, (legacy, record) in case.forms(out).items():
        pair = []
        for call in (legacy, lambda: case.lib.ia2p_unet_forward_x(case.net._ctx, case.ffi.current_stream(), record, case.ffi.ptr(case.ws), case.ws.numel())):
            out.fill_(float("nan"))
            assert call() == 0, (name, case.lib.ia2p_last_error(case.net._ctx))
            torch.cuda.synchronize()
            pair.append(out.clone())
        assert bool(torch.isfinite(pair[0].float()).all()), name
        assert torch.equal(*pair), f"ia2p_unet_forward{'' if name == 'forward' else '_' + name} and its record give other bytes"
        got[name] = pair[0]
    assert torch.equal(got["forward"], got["kv"])      # (tests/test_unet_gpu.py: the cached projections are the step's own, to the bit)
    assert len({bytes(t.cpu().numpy().tobytes()) for t in got.values()}) == 4, "an option did not reach the pass"


def test_record_size_is_checked(case):
    """a struct_size below the record as first published or above the library's own: IA2P_ERR_INVALID before any launch"""
    out = torch.zeros(B, 4, H, H, dtype=torch.half, device=DEV)
    record = case.forms(out)["forward"][1]
    for size in (0, C.sizeof(case.ffi.UNetCallC) - 8, C.sizeof(case.ffi.UNetCallC) + 8):
        record.struct_size = size
        assert case.lib.ia2p_unet_forward_x(case.net._ctx, case.ffi.current_stream(), record, case.ffi.ptr(case.ws), case.ws.numel()) == 1
        assert b"struct_size" in case.lib.ia2p_last_error(case.net._ctx) and case.lib.ia2p_workspace_bytes_x(case.net._ctx, record) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
