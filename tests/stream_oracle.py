"""TEST INFRASTRUCTURE — fp64 restatement of the streaming step (csrc/stream.hip, ganffn_encoder_stream_step,
gan_ffn_amd/streaming.py): per-layer K / V lists per cache slot, the slot / pos indirection, the skip rule and reset, built on the
row-wise pieces of oracle.ganffn_oracle (layer_norm, gelu, pe_table).  A step takes n rows, row i the next utterance of the dialogue
in slot slots[i]; nothing here looks at a dialogue as a whole, which is what the tests compare it with (O.encoder_stack /
O.gan_ffn_forward under causal_oracle.causal_attention on each dialogue alone).

Also the staggered schedule that the CPU and the GPU tests share."""
import math

import torch

from oracle import ganffn_oracle as O

LAYER_KEYS = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
              "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
              "norm2.bias"]


def layer_shapes(E, F):
    return [(3 * E, E), (3 * E,), (E, E), (E,), (F, E), (F,), (E, F), (E,), (E,), (E,), (E,), (E,)]


def random_stack_params(E, F, L, seed, head=None):
    """seeded fp64 parameter dict of a stack under the reference's state_dict keys; head = (D1, D2) adds fc1 / fc2"""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for l in range(L):
        for key, shape in zip(LAYER_KEYS, layer_shapes(E, F)):
            t = (torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5) * 0.4
            if key.startswith("norm") and key.endswith("weight"):
                t = t + 1.0
            P["transformer_encoder.layers.%d.%s" % (l, key)] = t
    if head is not None:
        D1, D2 = head
        for name, shape in (("fc1.weight", (D1, E)), ("fc1.bias", (D1,)), ("fc2.weight", (D2, D1)), ("fc2.bias", (D2,))):
            P[name] = (torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5) * 0.4
    return P


class StreamStack:
    """one encoder stack as a stream: K[l][s] / V[l][s] are the cached rows of layer l, slot s (position = list index)"""

    def __init__(self, P, H, n_layers, capacity, max_len=O.MAX_LEN, pe=None):
        self.P, self.H, self.L, self.capacity, self.max_len = P, H, n_layers, capacity, max_len
        self.E = P["transformer_encoder.layers.0.self_attn.out_proj.weight"].shape[0]
        if pe is None:
            pe = P["position_encoding.pe"] if "position_encoding.pe" in P else O.pe_table(self.E, dtype=torch.float64)
        self.pe = pe.reshape(-1, self.E).double()
        self.K = [[[] for _ in range(capacity)] for _ in range(n_layers)]
        self.V = [[[] for _ in range(capacity)] for _ in range(n_layers)]
        self.pos = [0] * capacity

    def live(self, s):
        return 0 <= s < self.capacity and 0 <= self.pos[s] < self.max_len

    def reset(self, slots=None):
        """positions back to 0 (the lists are cut there: what lay behind a position is never read)"""
        for s in (range(self.capacity) if slots is None else slots):
            self.pos[s] = 0
            for l in range(self.L):
                del self.K[l][s][:]
                del self.V[l][s][:]

    def advance(self, slots):
        for s in slots:
            if self.live(s):
                self.pos[s] += 1

    def pe_gather(self, x, slots):
        """x0[i] = x[i] + pe[pos[slots[i]]]; a skipped row gives a zero row"""
        out = torch.zeros_like(x)
        for i, s in enumerate(slots):
            if self.live(s):
                out[i] = x[i] + self.pe[self.pos[s]]
        return out

    def attention(self, l, qkv, slots):
        """append the rows' K / V at their positions and attend with their Q over keys 0 .. pos -> o [n, E]; a row whose slot
        is out of range or whose position is outside [0, max_len) is skipped: zeros, cache untouched"""
        E, H = self.E, self.H
        hd = E // H
        o = torch.zeros(qkv.shape[0], E, dtype=qkv.dtype)
        for i, s in enumerate(slots):
            if not self.live(s):
                continue
            t = self.pos[s]
            K, V = self.K[l][s], self.V[l][s]
            assert len(K) >= t and len(V) >= t, "position ahead of the cache"
            del K[t:]
            del V[t:]
            K.append(qkv[i, E:2 * E].clone())
            V.append(qkv[i, 2 * E:].clone())
            q = qkv[i, :E].reshape(H, hd)
            k = torch.stack(K).reshape(t + 1, H, hd)
            v = torch.stack(V).reshape(t + 1, H, hd)
            sc = torch.einsum("hd,jhd->hj", q, k) * (1.0 / math.sqrt(hd))
            p = torch.softmax(sc, dim=-1)
            o[i] = torch.einsum("hj,jhd->hd", p, v).reshape(E)
        return o

    def step(self, x, slots):
        """x [n, E] -> the stack's output rows [n, E] (eval).  Does NOT advance the positions (advance(slots) does)."""
        P = self.P
        x = self.pe_gather(x.double(), slots)
        for l in range(self.L):
            pre = "transformer_encoder.layers.%d." % l
            qkv = x @ P[pre + "self_attn.in_proj_weight"].T + P[pre + "self_attn.in_proj_bias"]
            a = self.attention(l, qkv, slots)
            a = a @ P[pre + "self_attn.out_proj.weight"].T + P[pre + "self_attn.out_proj.bias"]
            x = O.layer_norm(x + a, P[pre + "norm1.weight"], P[pre + "norm1.bias"])
            h = torch.relu(x @ P[pre + "linear1.weight"].T + P[pre + "linear1.bias"])
            y = h @ P[pre + "linear2.weight"].T + P[pre + "linear2.bias"]
            x = O.layer_norm(x + y, P[pre + "norm2.weight"], P[pre + "norm2.bias"])
        return x


class StreamClassifier:
    """GAN_FFN as a stream: three generator stacks with their GELU heads, the sum, fc, log_softmax — and one position per slot"""

    def __init__(self, gen_params, heads, n_layers, fc_w, fc_b, capacity, max_len=O.MAX_LEN):
        """gen_params: {"acoustic" | "visual" | "text": parameter dict with fc1 / fc2}; heads: {name: H}"""
        self.stacks = {k: StreamStack(gen_params[k], heads[k], n_layers, capacity, max_len) for k in ("acoustic", "visual", "text")}
        self.fc_w, self.fc_b = fc_w.double(), fc_b.double()

    def reset(self, slots=None):
        for st in self.stacks.values():
            st.reset(slots)

    def step(self, acoustic, visual, text, slots):
        fusion = 0
        for k, x in (("acoustic", acoustic), ("visual", visual), ("text", text)):
            st = self.stacks[k]
            t = O.gelu(st.step(x, slots))
            t = O.gelu(t @ st.P["fc1.weight"].T + st.P["fc1.bias"])
            t = O.gelu(t @ st.P["fc2.weight"].T + st.P["fc2.bias"])
            fusion = fusion + t
        for st in self.stacks.values():
            st.advance(slots)
        return torch.log_softmax(fusion @ self.fc_w.T + self.fc_b, dim=1)


# ----------------------------------------------------------------------------------------------------------------
# the staggered schedule: (slot, first step, length) per dialogue
# ----------------------------------------------------------------------------------------------------------------
# capacity 4; dialogues of 66, 40, 1 and 17 utterances that start at different steps; slot 2 is reset after its one-utterance
# dialogue and reused for a fifth; steps with n = 1, 2, 3 (< capacity) and n = 4
STAGGERED = [(0, 0, 66), (1, 3, 40), (2, 5, 1), (3, 7, 17), (2, 9, 6)]
# the session test's: capacity 3, dialogues of 9, 1 and 5 utterances
SHORT = [(0, 0, 9), (1, 2, 1), (2, 3, 5)]


def schedule(dialogues, rotate=True):
    """-> events in order: ("reset", [slots]) before a slot's second dialogue, ("step", [(dialogue, t), ...], [slots]) with the
    active dialogues' next utterances; the row order rotates from step to step so that a dialogue does not keep its row"""
    events = []
    used = set()
    last = max(a + n for _, a, n in dialogues)
    for k in range(last):
        starting = [d for d, (s, a, n) in enumerate(dialogues) if a == k]
        again = [dialogues[d][0] for d in starting if dialogues[d][0] in used]
        if again:
            events.append(("reset", again))
        used |= {dialogues[d][0] for d in starting}
        rows = [(d, k - a) for d, (s, a, n) in enumerate(dialogues) if a <= k < a + n]
        if not rows:
            continue
        if rotate:
            r = k % len(rows)
            rows = rows[r:] + rows[:r]
        events.append(("step", rows, [dialogues[d][0] for d, _ in rows]))
    return events
