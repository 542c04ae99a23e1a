"""The oracle with key lengths: `with masked_attention(lengths):` swaps oracle.ganffn_oracle.attention for a restatement in
which dialogue b attends over its first lengths[b] keys only — the scores of keys j >= lengths[b] are -inf before the softmax,
which is what nn.TransformerEncoder(..., src_key_padding_mask = (j >= lengths[b])) computes.  The dropout keep mask is the
contract's (philox.attn_keep_mask: it does not depend on lengths), applied after the masked softmax.  Everything built on
O.attention (O.encoder_stack, engine_oracle.phase2_step / drnn_step) becomes its masked form inside the block, and oracle/
stays as it is (tests/test_hip_ops.py swaps O.ENC_DROPOUT the same way)."""
import contextlib
import math

import numpy as np
import torch

from oracle import ganffn_oracle as O
from oracle import philox


def _masked_attention(lengths):
    lengths = [int(n) for n in lengths]

    def attention(qkv, B, H, layer, rng=None):
        S = qkv.shape[0]
        E = qkv.shape[2] // 3
        hd = E // H
        lens = lengths
        if rng is not None and getattr(rng, "select", None) is not None and len(lens) == rng.full_batch:
            lens = [lens[i] for i in rng.select]
        assert len(lens) == B, (len(lens), B)
        n = torch.tensor([min(max(v, 1), S) for v in lens])                       # the kernels' clamp
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]

        def heads(t):  # (S, B, E) -> (B*H, S, hd)
            return t.reshape(S, B * H, hd).transpose(0, 1)

        q, k, v = heads(q), heads(k), heads(v)
        # padded keys: out of the scores AND out of the value product (a finite value at a padded row changes nothing)
        dead = (torch.arange(S).unsqueeze(0) >= n.unsqueeze(1)).repeat_interleave(H, 0)        # (B*H, S) key j is padding
        s = torch.matmul(q, k.transpose(1, 2)) * (1.0 / math.sqrt(hd))
        s = s.masked_fill(dead.unsqueeze(1), float("-inf"))
        p = torch.softmax(s, dim=-1)
        if rng is not None and rng.train:
            if getattr(rng, "select", None) is not None:
                full = philox.attn_keep_mask(rng.full_batch, H, S, O.ENC_DROPOUT, O.SITE_LAYER0 + 4 * layer + 0, rng.seed, rng.offset)
                keep = torch.from_numpy(np.ascontiguousarray(full.reshape(rng.full_batch, H, S, S)[rng.select].reshape(B * H, S, S)))
            else:
                keep = torch.from_numpy(philox.attn_keep_mask(B, H, S, O.ENC_DROPOUT, O.SITE_LAYER0 + 4 * layer + 0,
                                                              rng.seed, rng.offset))
            p = p * keep.to(p.dtype) * (1.0 / (1.0 - O.ENC_DROPOUT))
        o = torch.matmul(p, v.masked_fill(dead.unsqueeze(2), 0.0))
        return o.transpose(0, 1).reshape(S, B, E)

    return attention


@contextlib.contextmanager
def masked_attention(lengths):
    """inside the block O.attention ignores keys j >= lengths[b] of dialogue b (lengths clamped to [1, S])"""
    saved = O.attention
    O.attention = _masked_attention(lengths)
    try:
        yield
    finally:
        O.attention = saved


def masked_lse(qkv, B, H, lengths):
    """fp64 log-sum-exp over the valid keys of every (dialogue, head, query) score row -> (B*H, S)"""
    S, E = qkv.shape[0], qkv.shape[2] // 3
    hd = E // H
    n = torch.tensor([min(max(int(v), 1), S) for v in lengths])
    q = qkv[..., :E].double().reshape(S, B * H, hd).transpose(0, 1)
    k = qkv[..., E:2 * E].double().reshape(S, B * H, hd).transpose(0, 1)
    dead = (torch.arange(S).unsqueeze(0) >= n.unsqueeze(1)).repeat_interleave(H, 0)
    s = (q @ k.transpose(1, 2) / hd ** 0.5).masked_fill(dead.unsqueeze(1), float("-inf"))
    return torch.logsumexp(s, dim=-1)


def valid_rows(S, lengths):
    """(S, B) bool: position s of dialogue b is a real utterance"""
    return torch.arange(S).unsqueeze(1) < torch.as_tensor(lengths).unsqueeze(0)
