"""The oracle side of tests/test_region_unet_gpu.py: a regional IP-Adapter processor for the CPU oracle UNet, the formula of `ia2p_attention_regions` written with
plain torch softmaxes in the caller's dtype (in the manner of oracle/attn_processors_ref.py, which it does not edit):

    out = softmax(q k_text^T / sqrt(d)) v_text + sum_g scale * m_g * softmax(q k_ip[g]^T / sqrt(d)) v_ip[g]          group g = image-token rows 4 g .. 4 g + 3

`BasicTransformerBlock.forward` passes no keyword on, so the masks ride as an attribute of a holder every processor shares: `holder.masks` [G, h, w] or
[B, G, h, w] on the latent grid, pooled to the site's token count by the mean over f x f blocks -- what `ia2p_region_levels` computes."""
import torch

from oracle.attn_processors_ref import IPAttnProcessor2_0Ref, _sdpa, _split_heads


class Regions:
    """the masks of the forward that is running, shared by all processors of a network"""
    masks = None


def pool(masks, n_tokens):
    """[B, G, h, w] -> [B, G, n_tokens]: block mean by the factor that brings h w to n_tokens"""
    B, G, h, w = masks.shape
    f = next(f for f in (1, 2, 4, 8) if h % f == 0 and w % f == 0 and (h // f) * (w // f) == n_tokens)
    return torch.nn.functional.avg_pool2d(masks.reshape(B * G, 1, h, w), f).reshape(B, G, n_tokens)


class RegionalIPAttnProcessorRef(IPAttnProcessor2_0Ref):
    def __init__(self, plain: IPAttnProcessor2_0Ref, holder: Regions):
        torch.nn.Module.__init__(self)
        self.hidden_size, self.cross_attention_dim, self.scale = plain.hidden_size, plain.cross_attention_dim, plain.scale
        self.to_k_ip, self.to_v_ip = plain.to_k_ip, plain.to_v_ip
        self.holder = holder

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, *a, **kw):
        b, nq, _ = hidden_states.shape
        m = self.holder.masks.to(hidden_states.dtype)
        if m.ndim == 3:
            m = m[None].expand(b, *m.shape)
        m = pool(m, nq)                                                     # [b, G, nq]
        G = m.shape[1]
        q = attn.to_q(hidden_states)
        end = encoder_hidden_states.shape[1] - 4 * G
        text, ip = encoder_hidden_states[:, :end], encoder_hidden_states[:, end:]
        qh = _split_heads(q, b, attn.heads)
        o = _sdpa(qh, _split_heads(attn.to_k(text), b, attn.heads), _split_heads(attn.to_v(text), b, attn.heads))
        ipk, ipv = _split_heads(self.to_k_ip(ip), b, attn.heads), _split_heads(self.to_v_ip(ip), b, attn.heads)
        for g in range(G):                                                  # every group its own softmax over its four keys, weighted per query
            og = _sdpa(qh, ipk[:, :, 4 * g:4 * g + 4], ipv[:, :, 4 * g:4 * g + 4])
            o = o + self.scale * m[:, g].reshape(b, 1, nq, 1) * og
        o = o.transpose(1, 2).reshape(b, -1, q.shape[-1]).to(q.dtype)
        o = attn.to_out[1](attn.to_out[0](o))
        if attn.residual_connection:
            o = o + hidden_states
        return o / attn.rescale_output_factor


def build_regional_unet(oracle, cfg, sd, ip_state, ip_scale):
    """the oracle UNet with the regional processor on every attn2 (installed through set_attn_processor) -> (net, holder)"""
    net = oracle.build_unet(cfg, sd, ip_state, ip_scale=ip_scale)
    holder = Regions()
    procs = {n: (RegionalIPAttnProcessorRef(p, holder) if isinstance(p, IPAttnProcessor2_0Ref) else p) for n, p in net.attn_processors.items()}
    net.set_attn_processor(procs)
    return net.eval(), holder
