"""The oracle with causal self-attention: `with causal_attention(lengths=None):` swaps oracle.ganffn_oracle.attention for a
restatement in which query i of dialogue b attends to keys j <= i and, when lengths are given, j < clamp(lengths[b], 1, S) — the
scores of every other key are -inf before the softmax, which is what nn.TransformerEncoder(src, mask = triu(-inf, 1),
src_key_padding_mask = (j >= lengths[b])) computes.  The dropout keep mask is the contract's (philox.attn_keep_mask: it depends
on neither mask), applied after the masked softmax.  Everything built on O.attention (O.encoder_stack, engine_oracle.phase2_step)
becomes its causal form inside the block, and oracle/ stays as it is (tests/key_len_oracle.py does the same for lengths alone)."""
import contextlib
import math

import numpy as np
import torch

from oracle import ganffn_oracle as O
from oracle import philox


def dead_keys(S, B, H, lengths):
    """(B*H, S, S) bool: key j is masked for query i — j > i, or j at or past the dialogue's clamped length"""
    n = torch.full((B,), S) if lengths is None else torch.tensor([min(max(int(v), 1), S) for v in lengths])
    assert n.numel() == B, (n.numel(), B)
    pad = (torch.arange(S).unsqueeze(0) >= n.unsqueeze(1)).repeat_interleave(H, 0)              # (B*H, S)
    future = torch.triu(torch.ones(S, S, dtype=torch.bool), 1)                                  # (query, key)
    return pad.unsqueeze(1) | future.unsqueeze(0)


def _causal_attention(lengths):
    lengths = None if lengths is None else [int(n) for n in lengths]

    def attention(qkv, B, H, layer, rng=None):
        S = qkv.shape[0]
        E = qkv.shape[2] // 3
        hd = E // H
        lens = lengths
        if lens is not None and rng is not None and getattr(rng, "select", None) is not None and len(lens) == rng.full_batch:
            lens = [lens[i] for i in rng.select]
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]

        def heads(t):  # (S, B, E) -> (B*H, S, hd)
            return t.reshape(S, B * H, hd).transpose(0, 1)

        q, k, v = heads(q), heads(k), heads(v)
        dead = dead_keys(S, B, H, lens)
        s = torch.matmul(q, k.transpose(1, 2)) * (1.0 / math.sqrt(hd))
        p = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
        if rng is not None and rng.train:
            if getattr(rng, "select", None) is not None:
                full = philox.attn_keep_mask(rng.full_batch, H, S, O.ENC_DROPOUT, O.SITE_LAYER0 + 4 * layer + 0, rng.seed, rng.offset)
                keep = torch.from_numpy(np.ascontiguousarray(full.reshape(rng.full_batch, H, S, S)[rng.select].reshape(B * H, S, S)))
            else:
                keep = torch.from_numpy(philox.attn_keep_mask(B, H, S, O.ENC_DROPOUT, O.SITE_LAYER0 + 4 * layer + 0,
                                                              rng.seed, rng.offset))
            p = p * keep.to(p.dtype) * (1.0 / (1.0 - O.ENC_DROPOUT))
        # a key that no query of the dialogue may see is out of the value product too (a finite value there changes nothing)
        o = torch.matmul(p, v.masked_fill(dead.all(dim=1).unsqueeze(2), 0.0))
        return o.transpose(0, 1).reshape(S, B, E)

    return attention


@contextlib.contextmanager
def causal_attention(lengths=None):
    """inside the block O.attention is causal (keys j <= i), over the first lengths[b] keys of dialogue b when lengths are given"""
    saved = O.attention
    O.attention = _causal_attention(lengths)
    try:
        yield
    finally:
        O.attention = saved


def causal_lse(qkv, B, H, lengths=None):
    """fp64 log-sum-exp over the allowed keys of every (dialogue, head, query) score row -> (B*H, S)"""
    S, E = qkv.shape[0], qkv.shape[2] // 3
    hd = E // H
    q = qkv[..., :E].double().reshape(S, B * H, hd).transpose(0, 1)
    k = qkv[..., E:2 * E].double().reshape(S, B * H, hd).transpose(0, 1)
    s = (q @ k.transpose(1, 2) / hd ** 0.5).masked_fill(dead_keys(S, B, H, lengths), float("-inf"))
    return torch.logsumexp(s, dim=-1)
