"""Word-level stand-in for the LLM's LlamaTokenizer (its sentencepiece model is checkpoint data that is not available here), with the special
tokens the reference adds on top of the base vocabulary (llm/model/any2pix_arch.py:285-288). `forward_llm` needs `tokenizer(text).input_ids`,
`tokenizer(text, return_tensors='pt').input_ids`, `add_special_tokens=False`, `bos_token_id` and `batch_decode`."""
import re
import types
import zlib

import torch

ADDED_TOKENS = ["<im_gen_start>", "<im_gen>", "<mask_gen>", "<audio_gen>", "<audio_gen_start>", "<audio>", "<video>", "<base>", "<base_null>"]


class StubLlamaTokenizer:
    """ids: 0 <unk>, 1 <s>, 2 </s>, words hashed into [3, base_vocab), the added tokens at base_vocab .. base_vocab + 8.
    Text is split at whitespace and around special tokens; decoding joins with single spaces (ids never seen decode as `w<id>`)."""
    bos_token_id, eos_token_id, unk_token_id = 1, 2, 0

    def __init__(self, base_vocab=503):
        self.base_vocab = base_vocab
        self.special = {"<unk>": 0, "<s>": 1, "</s>": 2}
        self.special.update({t: base_vocab + i for i, t in enumerate(ADDED_TOKENS)})
        self.words = {}
        self._split = re.compile("(" + "|".join(re.escape(t) for t in sorted(self.special, key=len, reverse=True)) + ")")

    def __len__(self):
        return self.base_vocab + len(ADDED_TOKENS)

    def _word_id(self, w):
        i = 3 + zlib.crc32(w.encode()) % (self.base_vocab - 3)
        self.words.setdefault(i, w)
        return i

    def encode(self, text, add_special_tokens=True):
        ids = [self.bos_token_id] if add_special_tokens else []
        for piece in self._split.split(text):
            if piece in self.special:
                ids.append(self.special[piece])
            else:
                ids += [self._word_id(w) for w in piece.split()]
        return ids

    def __call__(self, text, return_tensors=None, add_special_tokens=True):
        ids = self.encode(text, add_special_tokens)
        if return_tensors == "pt":
            return types.SimpleNamespace(input_ids=torch.tensor([ids], dtype=torch.long))
        return types.SimpleNamespace(input_ids=ids)

    def batch_decode(self, ids, skip_special_tokens=False):
        inv = {v: k for k, v in self.special.items()}
        out = []
        for row in ids:
            toks = []
            for i in (row.tolist() if hasattr(row, "tolist") else row):
                if i in inv:
                    if not skip_special_tokens:
                        toks.append(inv[i])
                else:
                    toks.append(self.words.get(i, f"w{i}"))
            out.append(" ".join(toks))
        return out
