"""fp64 restatement of the streamed DialogueRNN head (csrc/drnn_stream.hip, streaming.DrnnStreamSession): ONE recurrence step over
explicit G / Q / E arrays in the layout include/ganffn.h documents, the single-query general2 attention over a slot's emotion
history, and the classifier tail on top.  Written from the definition (DialogueRNNCell.forward for one real utterance, eval mode)
with the cell's parameter tensors and plain matrix products; it calls neither the cell's forward nor a HIP kernel.  What it is
compared with: drnn_causal_oracle.uni_head run on each dialogue ALONE."""
import torch

NAN = float("nan")


def a4(k):
    return (k + 3) & ~3


def _gru(x, h, wih, whh, bih, bhh):
    """torch.nn.GRUCell on rows: r, z, n row blocks"""
    gi, gh = x @ wih.T + bih, h @ whh.T + bhh
    W = h.shape[-1]
    r = torch.sigmoid(gi[..., :W] + gh[..., :W])
    z = torch.sigmoid(gi[..., W:2 * W] + gh[..., W:2 * W])
    n = torch.tanh(gi[..., 2 * W:] + r * gh[..., 2 * W:])
    return (1 - z) * n + z * h


def att_type(cell):
    return "simple" if type(cell.attention).__name__ == "SimpleAttention" else cell.attention.att_type


def context(cell, u, hist):
    """c_t of one dialogue: hist (t, D_g) = g_0 .. g_{t-1}, u (D_m); zeros without history"""
    if hist.shape[0] == 0:
        return u.new_zeros(cell.D_g)
    kind, a = att_type(cell), cell.attention
    if kind == "simple":
        s = hist @ a.scalar.weight[0]
    elif kind == "dot":
        s = hist @ u
    elif kind == "general":
        s = hist @ (a.transform.weight @ u)
    elif kind == "general2":
        s = torch.tanh(hist @ (a.transform.weight @ u + a.transform.bias))
    else:           # concat: memory columns first
        W, Dg = a.transform.weight, cell.D_g
        s = torch.tanh(hist @ W[:, :Dg].T + W[:, Dg:] @ u) @ a.vector_prod.weight[0]
    return torch.softmax(s, 0) @ hist


def general2_row(x, mem):
    """alpha_k = softmax_k(tanh(<x, e_k>)), att = sum_k alpha_k e_k over mem (nk, D) -> (att (D), alpha (nk))"""
    alpha = torch.softmax(torch.tanh(mem @ x), 0)
    return alpha @ mem, alpha


class HeadState:
    """G [capacity][max_len][H], Q [capacity][parties][H], E [capacity][max_len][He] (fp64); NaN where nothing was written"""

    def __init__(self, cell, capacity, max_len, parties):
        self.cell, self.capacity, self.max_len, self.parties = cell, capacity, max_len, parties
        H, He = cell.D_g, cell.D_e
        self.G = torch.full((capacity, max_len, H), NAN, dtype=torch.float64)
        self.Q = torch.full((capacity, parties, H), NAN, dtype=torch.float64)
        self.E = torch.full((capacity, max_len, He), NAN, dtype=torch.float64)

    def clone(self):
        c = HeadState(self.cell, self.capacity, self.max_len, self.parties)
        c.G, c.Q, c.E = self.G.clone(), self.Q.clone(), self.E.clone()
        return c

    def offsets(self):
        """(G, Q, E, total) float offsets of the flat state: each region rounded up to a multiple of 4 floats"""
        q = a4(self.G.numel())
        e = q + a4(self.Q.numel())
        return 0, q, e, e + a4(self.E.numel())

    def flat(self, dtype=torch.float32, fill=NAN):
        g, q, e, total = self.offsets()
        out = torch.full((total,), fill, dtype=dtype)
        out[g:g + self.G.numel()] = self.G.reshape(-1).to(dtype)
        out[q:q + self.Q.numel()] = self.Q.reshape(-1).to(dtype)
        out[e:e + self.E.numel()] = self.E.reshape(-1).to(dtype)
        return out

    def poison(self, pos):
        """NaN at and above every slot's position (and every party row of a slot at position 0): what a step must not read"""
        for s, t in enumerate(pos):
            t = max(0, min(int(t), self.max_len))
            self.G[s, t:] = NAN
            self.E[s, t:] = NAN
            if t == 0:
                self.Q[s] = NAN

    def live(self, s, t, sp, off, count_i):
        return (0 <= s < self.capacity and t >= 0 and t + off < self.max_len and 0 <= sp < self.parties
                and (count_i is None or off < count_i))

    @torch.no_grad()
    def step(self, U, spk, slots, pos, off=0, count=None):
        """rows U (n, D_m), speakers spk, slot list, positions per SLOT (not advanced) -> e_out (n, D_e); skipped rows are zero
        rows and leave the state alone"""
        c = self.cell
        out = torch.zeros(len(slots), c.D_e, dtype=torch.float64)
        for i, s in enumerate(slots):
            p0 = pos[s] if 0 <= s < self.capacity else -1
            if not self.live(s, p0, spk[i], off, None if count is None else count[i]):
                continue
            t, sp, u = p0 + off, spk[i], U[i].to(torch.float64)
            first = t == 0
            q = torch.zeros(self.parties, c.D_g, dtype=torch.float64) if first else self.Q[s].clone()
            g_prev = torch.zeros(c.D_g, dtype=torch.float64) if first else self.G[s, t - 1]
            e_prev = torch.zeros(c.D_e, dtype=torch.float64) if first else self.E[s, t - 1]
            g = _gru(torch.cat([u, q[sp]]), g_prev, c.g_cell.weight_ih, c.g_cell.weight_hh, c.g_cell.bias_ih, c.g_cell.bias_hh)
            ctx = context(c, u, self.G[s, :t])
            qs = _gru(torch.cat([u, ctx]), q[sp], c.p_cell.weight_ih, c.p_cell.weight_hh, c.p_cell.bias_ih, c.p_cell.bias_hh)
            if c.listener_state:
                x = torch.cat([u, qs]).unsqueeze(0).expand(self.parties, -1)
                qn = _gru(x, q, c.l_cell.weight_ih, c.l_cell.weight_hh, c.l_cell.bias_ih, c.l_cell.bias_hh)
            else:
                qn = q.clone()
            qn[sp] = qs
            e = _gru(qs, e_prev, c.e_cell.weight_ih, c.e_cell.weight_hh, c.e_cell.bias_ih, c.e_cell.bias_hh)
            self.G[s, t], self.Q[s], self.E[s, t] = g, qn, e
            out[i] = e
        return out

    @torch.no_grad()
    def extend(self, U, spk, slots, pos, count):
        """U (m, n, D_m), spk [m][n]: the step with off = 0 .. m-1 -> e_out (m, n, D_e)"""
        return torch.stack([self.step(U[j], spk[j], slots, pos, j, count) for j in range(U.shape[0])])


class StreamUni:
    """the streamed UniModel head: HeadState + positions + the tail (transform, general2 over E[s][0 .. t], linear, ReLU,
    smax_fc, log_softmax); the generators are not its business: it is fed fusion rows"""

    def __init__(self, um, capacity, max_len=110, parties=2):
        self.um = um
        self.state = HeadState(um.dialog_rnn_f.dialogue_cell, capacity, max_len, parties)
        self.pos = [0] * capacity
        self.poison = False

    def reset(self, slots=None):
        for s in (range(len(self.pos)) if slots is None else slots):
            self.pos[s] = 0

    @torch.no_grad()
    def _tail(self, e, s, t):
        um = self.um
        att, _ = general2_row(um.matchatt.transform.weight @ e + um.matchatt.transform.bias, self.state.E[s, :t + 1])
        h = torch.relu(um.linear.weight @ att + um.linear.bias)
        return torch.log_softmax(um.smax_fc.weight @ h + um.smax_fc.bias, 0)

    def step(self, fusion, spk, slots):
        if self.poison:
            self.state.poison(self.pos)
        e = self.state.step(fusion, spk, slots, self.pos)
        out = torch.stack([self._tail(e[i], s, self.pos[s]) for i, s in enumerate(slots)])
        for s in slots:
            self.pos[s] += 1
        return out

    def extend(self, fusion, spk, lengths, slots):
        """fusion (m, n, D_m) -> log_prob (m, n, C); rows past a length are NaN"""
        if self.poison:
            self.state.poison(self.pos)
        e = self.state.extend(fusion, spk, slots, self.pos, lengths)
        m, n = fusion.shape[:2]
        out = torch.full((m, n, self.um.smax_fc.weight.shape[0]), NAN, dtype=torch.float64)
        for i, s in enumerate(slots):
            for j in range(lengths[i]):
                out[j, i] = self._tail(e[j, i], s, self.pos[s] + j)
        for s, c in zip(slots, lengths):
            self.pos[s] += c
        return out


def one_hot(spk, parties):
    """speaker indices (S,) -> qmask (S, 1, parties) fp64"""
    return torch.nn.functional.one_hot(torch.as_tensor(spk), parties).to(torch.float64).unsqueeze(1)
