"""TEST INFRASTRUCTURE — fp64 restatement of the packed-sequence LSTM rule of csrc/lstm.hip (ganffn_lstm_packed_* /
ganffn_lstm_stack_packed_*, include/ganffn.h); the product never imports this module.

oracle/lstm_oracle.py's structure with one addition.  lengths[b] is the number of real steps of dialogue b (<= 0: empty, > S: S).
In both directions, for dialogue b at time index t >= lengths[b], the step SELECTS c_t = 0 and h_t = 0 (torch.where, so the
row's values — and, under autograd, the upstream gradients at that position — are discarded, not multiplied by 0); at
t < lengths[b] the arithmetic is lstm_oracle's.  That is pack_padded_sequence -> nn.LSTM -> pad_packed_sequence(total_length = S):
tests/test_lstm_packed_cpu.py pins it to torch's packed nn.LSTM at 1e-12 (forward, dx, every parameter gradient, junk upstream
gradients at padded positions) and to LO.lstm_forward exactly at full lengths.  Train mode: the inter-layer dropout goes through
oracle.ganffn_oracle's Philox helpers exactly as in LO.lstm_forward (site SITE_LSTM + layer, one offset per call)."""
import torch

from oracle import ganffn_oracle as O
from oracle import lstm_oracle as LO

SITE_LSTM = LO.SITE_LSTM


def valid_mask(lengths, S):
    """(S, B, 1) bool: t < lengths[b]"""
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    return (torch.arange(S).unsqueeze(1) < lengths.unsqueeze(0)).unsqueeze(2)


def lstm_direction(x, lengths, w_ih, w_hh, b_ih, b_hh, reverse):
    """x (S, B, In) -> h (S, B, H) of one direction; zero state and zero output at t >= lengths[b]"""
    S, B, _ = x.shape
    H = w_hh.shape[1]
    valid = valid_mask(lengths, S)
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    zero = x.new_zeros(B, H)
    out = [None] * S
    xg = x @ w_ih.T + b_ih
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        G = xg[t] + h @ w_hh.T + b_hh
        i, f, g, o = torch.sigmoid(G[:, :H]), torch.sigmoid(G[:, H:2 * H]), torch.tanh(G[:, 2 * H:3 * H]), torch.sigmoid(G[:, 3 * H:])
        c = torch.where(valid[t], f * c + i * g, zero)
        h = torch.where(valid[t], o * torch.tanh(c), zero)
        out[t] = h
    return torch.stack(out, 0)


def lstm_forward(x, lengths, P, num_layers, p_drop=0.0, rng=None, prefix="", offsets=None):
    """LO.lstm_forward on packed sequences: pad_packed_sequence(nn.LSTM(...)(pack_padded_sequence(x, lengths)), total_length=S)[0].
    Same arguments otherwise (P: torch's parameter names -> tensors; rng: O.Rng; offsets: one Philox offset per dropout call)."""
    h = x
    for l in range(num_layers):
        f = lstm_direction(h, lengths, P[prefix + "weight_ih_l%d" % l], P[prefix + "weight_hh_l%d" % l], P[prefix + "bias_ih_l%d" % l],
                           P[prefix + "bias_hh_l%d" % l], False)
        b = lstm_direction(h, lengths, P[prefix + "weight_ih_l%d_reverse" % l], P[prefix + "weight_hh_l%d_reverse" % l],
                           P[prefix + "bias_ih_l%d_reverse" % l], P[prefix + "bias_hh_l%d_reverse" % l], True)
        h = torch.cat((f, b), dim=2)
        if l + 1 < num_layers and rng is not None and rng.train and p_drop > 0.0:
            off = offsets[l] if offsets is not None else rng.offset + l
            h = O._drop(h, p_drop, SITE_LSTM + l, rng.at(off))
    return h
