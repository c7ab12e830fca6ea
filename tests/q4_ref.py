"""CPU reference of the 4-bit weight format (include/ia2p.h, ia2p_llm_set_weight_format), in torch: the definition the HIP quantiser must
reproduce bit for bit. Blocks of 64 along the flattened tensor; absmax = max |w| as fp32; x = w / absmax in fp32; the code is the entry of
the (stably) sorted codebook at position #{thresholds strictly below x}, the thresholds being the fp32 midpoints of neighbouring entries;
an all-zero block stores absmax 0 and the code of x = 0. The dequantised weight is the fp32 product codebook[code] * absmax rounded to fp16.

The two tables are written from memory of bitsandbytes 0.41.2 and the QLoRA paper (neither package is needed or used here)."""
import torch

BLOCK = 64
CODEBOOKS = {
    "nf4": [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
            -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
            0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0],
    "fp4": [v / 12 for v in (0, 0.0625, 8, 12, 4, 6, 2, 3, -0.0, -0.0625, -8, -12, -4, -6, -2, -3)],
}


def sorted_codebook(codebook):
    """-> (sorted values fp32 [16], their codes [16], thresholds fp32 [15])"""
    s, order = torch.sort(torch.tensor(codebook, dtype=torch.float32), stable=True)
    return s, order, (s[:-1] + s[1:]) / 2


def quantize_ref(w, codebook):
    """fp16 [N, K] -> (codes uint8 [N, K], absmax fp32 [N * K / 64])"""
    assert w.dtype == torch.float16 and w.numel() % BLOCK == 0
    _, order, thr = sorted_codebook(codebook)
    blocks = w.float().reshape(-1, BLOCK)
    absmax = blocks.abs().amax(dim=1)
    x = torch.where(absmax[:, None] > 0, blocks / absmax[:, None], torch.zeros_like(blocks))
    pos = torch.bucketize(x, thr, right=False)           # = the number of thresholds strictly below x
    return order[pos].to(torch.uint8).reshape(w.shape), absmax


def dequantize_unrounded(codes, absmax, codebook):
    """the fp32 products codebook[code] * absmax, [N, K]"""
    cb = torch.tensor(codebook, dtype=torch.float32)
    return (cb[codes.long()].reshape(-1, BLOCK) * absmax[:, None]).reshape(codes.shape)


def dequantize_ref(codes, absmax, codebook):
    """-> fp16 [N, K]: the product rounded to the checkpoint dtype, as bitsandbytes hands it to the matmul"""
    return dequantize_unrounded(codes, absmax, codebook).half()


def round_trip(w, codebook):
    return dequantize_ref(*quantize_ref(w, codebook), codebook)
