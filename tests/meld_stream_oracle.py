"""TEST INFRASTRUCTURE — fp64 restatement of the streamed causal MELD classifier (csrc/lstm_stream.hip,
streaming.MeldStreamSession): ONE step of a forward-only nn.LSTM's layers over explicit Hs / Cs / E arrays in the layout
include/ganffn.h documents, and the streamed tail on top (matchatt.transform, the single-query general2 attention over a slot's
emotion history, hardswish(e + hardswish(att)), smax_fc, log-softmax).  Written from the definition (torch's LSTM cell, gate order
i, f, g, o) with the module's parameter tensors and plain matrix products; it calls neither nn.LSTM's forward nor a HIP kernel.
What it is compared with: meld_causal_oracle.forward run on each dialogue ALONE."""
import torch

from drnn_stream_oracle import a4, general2_row
from meld_step_oracle import hardswish

NAN = float("nan")


class LstmState:
    """Hs [capacity][L][H], Cs [capacity][L][H], E [capacity][max_len][H] (fp64); NaN where nothing was written.  lstm: an
    nn.LSTM(bidirectional=False) in fp64, read through weight_ih_l{k}, weight_hh_l{k}, bias_ih_l{k}, bias_hh_l{k}."""

    def __init__(self, lstm, capacity, max_len):
        self.lstm, self.capacity, self.max_len = lstm, capacity, max_len
        self.In, self.H, self.L = lstm.input_size, lstm.hidden_size, lstm.num_layers
        self.Hs = torch.full((capacity, self.L, self.H), NAN, dtype=torch.float64)
        self.Cs = torch.full((capacity, self.L, self.H), NAN, dtype=torch.float64)
        self.E = torch.full((capacity, max_len, self.H), NAN, dtype=torch.float64)

    def clone(self):
        c = LstmState(self.lstm, self.capacity, self.max_len)
        c.Hs, c.Cs, c.E = self.Hs.clone(), self.Cs.clone(), self.E.clone()
        return c

    def offsets(self):
        """(Hs, Cs, E, total) float offsets of the flat state: each region rounded up to a multiple of 4 floats"""
        c = a4(self.Hs.numel())
        e = c + a4(self.Cs.numel())
        return 0, c, e, e + a4(self.E.numel())

    def flat(self, dtype=torch.float32, fill=NAN):
        h, c, e, total = self.offsets()
        out = torch.full((total,), fill, dtype=dtype)
        out[h:h + self.Hs.numel()] = self.Hs.reshape(-1).to(dtype)
        out[c:c + self.Cs.numel()] = self.Cs.reshape(-1).to(dtype)
        out[e:e + self.E.numel()] = self.E.reshape(-1).to(dtype)
        return out

    def poison(self, pos):
        """NaN in E at and above every slot's position and in Hs / Cs of a slot at position 0: what a step must not read"""
        for s, t in enumerate(pos):
            t = max(0, min(int(t), self.max_len))
            self.E[s, t:] = NAN
            if t == 0:
                self.Hs[s] = NAN
                self.Cs[s] = NAN

    def live(self, s, t, off, count_i):
        return 0 <= s < self.capacity and t >= 0 and t + off < self.max_len and (count_i is None or off < count_i)

    @torch.no_grad()
    def step(self, x, slots, pos, off=0, count=None):
        """rows x (n, In), slot list, positions per SLOT (not advanced) -> e_out (n, H); skipped rows are zero rows and leave the
        state alone"""
        m = self.lstm
        out = torch.zeros(len(slots), self.H, dtype=torch.float64)
        for i, s in enumerate(slots):
            p0 = pos[s] if 0 <= s < self.capacity else -1
            if not self.live(s, p0, off, None if count is None else count[i]):
                continue
            t = p0 + off
            first = t == 0
            inp = x[i].to(torch.float64)
            for l in range(self.L):
                w_ih, w_hh = getattr(m, "weight_ih_l%d" % l), getattr(m, "weight_hh_l%d" % l)
                b_ih, b_hh = getattr(m, "bias_ih_l%d" % l), getattr(m, "bias_hh_l%d" % l)
                h_prev = torch.zeros(self.H, dtype=torch.float64) if first else self.Hs[s, l].clone()
                c_prev = torch.zeros(self.H, dtype=torch.float64) if first else self.Cs[s, l].clone()
                g = w_ih @ inp + b_ih + w_hh @ h_prev + b_hh
                H = self.H
                ig, fg, gg, og = torch.sigmoid(g[:H]), torch.sigmoid(g[H:2 * H]), torch.tanh(g[2 * H:3 * H]), torch.sigmoid(g[3 * H:])
                c = fg * c_prev + ig * gg
                h = og * torch.tanh(c)
                self.Hs[s, l], self.Cs[s, l] = h, c
                inp = h
            self.E[s, t] = inp
            out[i] = inp
        return out

    @torch.no_grad()
    def extend(self, x, slots, pos, count):
        """x (m, n, In): the step with off = 0 .. m-1 -> e_out (m, n, H)"""
        return torch.stack([self.step(x[j], slots, pos, j, count) for j in range(x.shape[0])])


class StreamMeld:
    """the streamed MELDLSTMModel(causal=True): LstmState + positions + the tail; model: the module in fp64"""

    def __init__(self, model, capacity, max_len=110):
        self.model = model
        self.state = LstmState(model.lstm, capacity, max_len)
        self.pos = [0] * capacity
        self.poison = False

    def reset(self, slots=None):
        for s in (range(len(self.pos)) if slots is None else slots):
            self.pos[s] = 0

    @torch.no_grad()
    def _tail(self, e, s, t):
        m = self.model
        att, _ = general2_row(m.matchatt.transform.weight @ e + m.matchatt.transform.bias, self.state.E[s, :t + 1])
        hidden = hardswish(e + hardswish(att))
        return torch.log_softmax(m.smax_fc.weight @ hidden + m.smax_fc.bias, 0)

    def step(self, text, slots):
        if self.poison:
            self.state.poison(self.pos)
        e = self.state.step(text, slots, self.pos)
        out = torch.stack([self._tail(e[i], s, self.pos[s]) for i, s in enumerate(slots)])
        for s in slots:
            self.pos[s] += 1
        return out

    def extend(self, text, lengths, slots):
        """text (m, n, D_m) -> log_prob (m, n, C); rows past a length are NaN"""
        if self.poison:
            self.state.poison(self.pos)
        e = self.state.extend(text, slots, self.pos, lengths)
        m, n = text.shape[:2]
        out = torch.full((m, n, self.model.smax_fc.weight.shape[0]), NAN, dtype=torch.float64)
        for i, s in enumerate(slots):
            for j in range(lengths[i]):
                out[j, i] = self._tail(e[j, i], s, self.pos[s] + j)
        for s, c in zip(slots, lengths):
            self.pos[s] += c
        return out


def alone(model, text):
    """meld_causal_oracle.forward on one dialogue alone: text (n, D_m) -> log_prob (n, C); model: the module in fp64"""
    import meld_causal_oracle as CO
    P = {k: v.detach().double() for k, v in model.state_dict().items()}
    n = text.shape[0]
    with torch.no_grad():
        return CO.forward(P, text.double().unsqueeze(1), torch.ones(1, n, dtype=torch.float64))[1][:, 0]
