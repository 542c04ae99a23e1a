"""TEST INFRASTRUCTURE — fp64 restatement of the stream prefill (csrc/stream.hip's chunk kernels, ganffn_encoder_stream_extend,
StreamSession.extend) on top of tests/stream_oracle.py: chunk i of a call holds counts[i] new rows of the dialogue in slot
slots[i], time-major [m, n, E]; row j attends over the slot's cached rows and the chunk's rows 0 .. j; the chunk skip rule.
Nothing here looks at a dialogue as a whole, which is what the tests compare it with."""
import math

import torch

from oracle import ganffn_oracle as O
import stream_oracle as SO


class ExtendStack(SO.StreamStack):
    """StreamStack with the chunk call; `step` and everything else are the parent's"""

    def chunk_live(self, s, c, m):
        """the skip rule of a chunk: slot in range, position not negative, 0 <= count <= m, and the chunk fits"""
        return 0 <= s < self.capacity and self.pos[s] >= 0 and 0 <= c <= m and self.pos[s] + c <= self.max_len

    def advance_chunks(self, slots, counts, m):
        for s, c in zip(slots, counts):
            if self.chunk_live(s, c, m):
                self.pos[s] += c

    def pe_gather_chunk(self, x, slots, counts):
        """x0[j, i] = x[j, i] + pe[pos[slots[i]] + j] for j < counts[i] of a live chunk; every other row is a zero row"""
        m = x.shape[0]
        out = torch.zeros_like(x)
        for i, (s, c) in enumerate(zip(slots, counts)):
            if self.chunk_live(s, c, m):
                t = self.pos[s]
                out[:c, i] = x[:c, i] + self.pe[t:t + c]
        return out

    def attention_chunk(self, l, qkv, slots, counts):
        """qkv [m, n, 3E] -> o [m, n, E]: the K / V of rows 0 .. c-1 are appended at the slot's position, row j attends over keys
        0 .. pos + j; rows j >= c and skipped chunks give zeros, and a skipped chunk leaves the cache alone.  Rows j >= c of qkv
        are not looked at."""
        E, H = self.E, self.H
        hd = E // H
        m = qkv.shape[0]
        o = torch.zeros(m, qkv.shape[1], E, dtype=qkv.dtype)
        for i, (s, c) in enumerate(zip(slots, counts)):
            if not self.chunk_live(s, c, m) or c == 0:
                continue
            t = self.pos[s]
            K, V = self.K[l][s], self.V[l][s]
            assert len(K) >= t and len(V) >= t, "position ahead of the cache"
            del K[t:]
            del V[t:]
            for j in range(c):
                K.append(qkv[j, i, E:2 * E].clone())
                V.append(qkv[j, i, 2 * E:].clone())
            k = torch.stack(K).reshape(t + c, H, hd)
            v = torch.stack(V).reshape(t + c, H, hd)
            for j in range(c):
                q = qkv[j, i, :E].reshape(H, hd)
                sc = torch.einsum("hd,jhd->hj", q, k[:t + j + 1]) * (1.0 / math.sqrt(hd))
                p = torch.softmax(sc, dim=-1)
                o[j, i] = torch.einsum("hj,jhd->hd", p, v[:t + j + 1]).reshape(E)
        return o

    def extend(self, x, slots, counts):
        """x [m, n, E] -> the stack's output rows [m, n, E] (eval); rows j >= counts[i] are meaningless.  Does NOT advance the
        positions (advance_chunks does)."""
        P = self.P
        x = self.pe_gather_chunk(x.double(), slots, counts)
        for l in range(self.L):
            pre = "transformer_encoder.layers.%d." % l
            qkv = x @ P[pre + "self_attn.in_proj_weight"].T + P[pre + "self_attn.in_proj_bias"]
            a = self.attention_chunk(l, qkv, slots, counts)
            a = a @ P[pre + "self_attn.out_proj.weight"].T + P[pre + "self_attn.out_proj.bias"]
            x = O.layer_norm(x + a, P[pre + "norm1.weight"], P[pre + "norm1.bias"])
            h = torch.relu(x @ P[pre + "linear1.weight"].T + P[pre + "linear1.bias"])
            y = h @ P[pre + "linear2.weight"].T + P[pre + "linear2.bias"]
            x = O.layer_norm(x + y, P[pre + "norm2.weight"], P[pre + "norm2.bias"])
        return x


class ExtendClassifier(SO.StreamClassifier):
    """StreamClassifier over ExtendStacks, with the chunk call"""

    def __init__(self, gen_params, heads, n_layers, fc_w, fc_b, capacity, max_len=O.MAX_LEN):
        self.stacks = {k: ExtendStack(gen_params[k], heads[k], n_layers, capacity, max_len) for k in ("acoustic", "visual", "text")}
        self.fc_w, self.fc_b = fc_w.double(), fc_b.double()

    def extend(self, acoustic, visual, text, slots, counts):
        """[m, n, *] inputs -> log_prob [m, n, n_classes]; advances the positions by counts"""
        fusion = 0
        for k, x in (("acoustic", acoustic), ("visual", visual), ("text", text)):
            st = self.stacks[k]
            t = O.gelu(st.extend(x, slots, counts))
            t = O.gelu(t @ st.P["fc1.weight"].T + st.P["fc1.bias"])
            t = O.gelu(t @ st.P["fc2.weight"].T + st.P["fc2.bias"])
            fusion = fusion + t
        for st in self.stacks.values():
            st.advance_chunks(slots, counts, acoustic.shape[0])
        return torch.log_softmax(fusion @ self.fc_w.T + self.fc_b, dim=-1)


# ----------------------------------------------------------------------------------------------------------------
# schedules that mix chunks and single steps
# ----------------------------------------------------------------------------------------------------------------
def pieces(n, split):
    """a dialogue of n rows cut as `split` says -> [(first row, rows)]"""
    assert sum(split) == n and all(c >= 1 for c in split)
    out, a = [], 0
    for c in split:
        out.append((a, c))
        a += c
    return out


# how each dialogue of SO.STAGGERED (66, 40, 1, 17 and 6 rows) is cut — a piece of one row is a step, a longer one a chunk — and the
# event round in which its first piece is due: dialogues 0 and 1 open together with chunks of 30 and 12 rows in one call, round 4
# has chunks of 33, 11 and 6 rows in one call, and slot 2 is reset for its second dialogue
STAGGERED_SPLITS = [[30, 1, 1, 1, 33], [12, 27, 1], [1], [5, 1, 11], [6]]
STAGGERED_STARTS = [0, 0, 1, 2, 4]


def mixed_schedule(dialogues, splits, starts):
    """-> events in order, from the (slot, _, rows) triples of a stream_oracle schedule, a split and a first round per dialogue:
    ("reset", [slots]) before a slot's second dialogue; ("extend", [(dialogue, first row, rows), ...], [slots]) for the pieces
    longer than one row that are due in a round; ("step", [(dialogue, row), ...], [slots]) for its one-row pieces.  Dialogue
    d's k-th piece is due in round starts[d] + k."""
    events, used = [], set()
    due = {}
    for d, ((s, _, n), sp) in enumerate(zip(dialogues, splits)):
        for k, (first, c) in enumerate(pieces(n, sp)):
            due.setdefault(starts[d] + k, []).append((d, first, c))
    for k in sorted(due):
        starting = [d for d, first, _ in due[k] if first == 0]
        again = [dialogues[d][0] for d in starting if dialogues[d][0] in used]
        if again:
            events.append(("reset", again))
        used |= {dialogues[d][0] for d in starting}
        chunks = [(d, first, c) for d, first, c in due[k] if c > 1]
        steps = [(d, first) for d, first, c in due[k] if c == 1]
        if chunks:
            events.append(("extend", chunks, [dialogues[d][0] for d, _, _ in chunks]))
        if steps:
            events.append(("step", steps, [dialogues[d][0] for d, _ in steps]))
    return events


def pad_chunks(xs, chunks, fill=0.0):
    """the time-major padded input [m, n, E] of an "extend" event from per-dialogue rows xs[d] [rows, E] -> (x, counts)"""
    counts = [c for _, _, c in chunks]
    m = max(counts)
    x = torch.full((m, len(chunks), xs[0].shape[1]), fill, dtype=xs[0].dtype, device=xs[0].device)
    for i, (d, first, c) in enumerate(chunks):
        x[:c, i] = xs[d][first:first + c]
    return x, counts
