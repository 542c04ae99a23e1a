"""Streaming causal classifier: label each utterance as it arrives.

`GAN_FFN(causal=True).stream(capacity, max_len)` returns a StreamSession.  Under the causal mask the K and V of a past utterance
never change and everything else in the classifier is row-wise (positional encoding, LayerNorm, FFN, the GELU head, the sum, `fc`,
log_softmax), so `step` runs the three generators on the NEW rows alone against per-layer K/V caches (csrc/stream.hip,
ganffn_encoder_stream_step) instead of on the whole prefix: constant rows and constant memory traffic per utterance.  A step's
values agree with the matching rows of the full causal forward to rounding, not bit for bit (the kernels' summation-order
rules are evaluated for n rows).  `extend` ingests several utterances per dialogue in one call (ganffn_encoder_stream_extend: one
causal pass over the new rows against the same caches) — a dialogue joined under way, caches rebuilt after the weights changed,
utterances that arrive in bursts.

`GAN_FFN_DialogueRNN(causal=True).stream(capacity, max_len, parties)` returns a DrnnStreamSession: the same generator caches plus
the DialogueRNN head's per-slot state (global history, party states, emotion history; csrc/drnn_stream.hip), one recurrence step
per new utterance.

`MELDLSTMModel(causal=True).stream(capacity, max_len)` returns a MeldStreamSession: no generators, the forward-only LSTM's per-slot
(h, c) of every layer and the emotion history (csrc/lstm_stream.hip), one LSTM step per new utterance.
"""
import torch

from . import ops
from .ops import MAX_DIALOGUES

GEN_NAMES = ("acoustic_generator", "visual_generator", "text_generator")


class _Bufs:
    """everything a step over n rows touches: allocated on the first step at that n, never again"""

    def __init__(self, sess, n):
        dev, f32 = sess.device, dict(device=sess.device, dtype=torch.float32)
        self.slot = torch.zeros(n, device=dev, dtype=torch.int32)       # the kernels' slot list
        self.slot64 = torch.zeros(n, device=dev, dtype=torch.int64)     # the same, as the index of the position advance
        self.ones = torch.ones(n, device=dev, dtype=torch.int32)
        self.slots_host = None                                          # what self.slot holds (tuple), to skip equal uploads
        self.x = [torch.zeros(n, g.d_model, **f32) for g in sess.gens]
        self.enc = [torch.empty(n, g.d_model, **f32) for g in sess.gens]
        self.head_cfg, self.head_saved, self.head_ws, self.head_out = [], [], [], []
        for g in sess.gens:
            hc = ops.head_cfg(n, g.d_model, g.fc1.weight.shape[0], g.fc2.weight.shape[0], 0, float(g.dropout.p), train=False)
            n_saved, n_ws = ops.head_sizes(hc)
            self.head_cfg.append(hc)
            self.head_saved.append(torch.empty(n_saved, **f32))
            self.head_ws.append(torch.empty(n_ws, **f32))
            self.head_out.append(torch.empty(n, g.fc2.weight.shape[0], **f32))
        self.fusion = torch.empty(n, sess._fusion_width(), **f32)
        self.logits = torch.empty(n, sess.net.n_classes, **f32)
        self.log_prob = torch.empty(n, sess.net.n_classes, **f32)
        self.graph = None
        self.graph_key = None


class _ExtBufs:
    """everything an extend over [m, n] touches: allocated on the first extend at that (m, n), never again.  One native call
    carries at most ops.STREAM_EXTEND_MAX_ROWS rows: the n dialogues run in groups of `per` columns (the last may be smaller),
    and the groups of one size share their row buffers (they run one after the other on one stream)."""

    def __init__(self, sess, m, n):
        dev = sess.device
        self.slot = torch.zeros(n, device=dev, dtype=torch.int32)
        self.slot64 = torch.zeros(n, device=dev, dtype=torch.int64)
        self.count = torch.zeros(n, device=dev, dtype=torch.int32)
        self.slots_host = self.counts_host = None                       # what the device copies hold, to skip equal uploads
        per = max(1, min(n, ops.STREAM_EXTEND_MAX_ROWS // m))
        self.groups = [(lo, min(lo + per, n)) for lo in range(0, n, per)]
        self.rows = {hi - lo: _Bufs(sess, m * (hi - lo)) for lo, hi in self.groups}      # (at most two sizes)
        self.ws = [torch.empty(ops.stream_extend_sizes(cfg, m * per), device=dev, dtype=torch.float32) for cfg in sess.cfgs]
        single = len(self.groups) == 1
        self.log_prob = (self.rows[n].log_prob.view(m, n, -1) if single else
                         torch.empty(m, n, sess.net.n_classes, device=dev, dtype=torch.float32))


class _SlotStream:
    """The slot and position bookkeeping every streaming session shares: `capacity` slots of up to `max_len` positions, the
    positions on the device (int32) with a host mirror that only step, extend and reset change, slot-list validation, reset, the
    slot upload of a call's buffers and the position advance."""

    @staticmethod
    def _check_capacity(capacity, max_len):
        """-> (capacity, max_len) as ints in range (max_len None: model.MAX_LEN), else ValueError"""
        from .model import MAX_LEN
        max_len = MAX_LEN if max_len is None else int(max_len)
        if not 1 <= int(capacity) <= MAX_DIALOGUES:
            raise ValueError("capacity=%r out of range [1, %d]" % (capacity, MAX_DIALOGUES))
        if not 1 <= max_len <= MAX_LEN:
            raise ValueError("max_len=%r out of range [1, %d] (PositionalEncoding max_len)" % (max_len, MAX_LEN))
        return int(capacity), max_len

    @staticmethod
    def _check_one_gpu(net, dev, what):
        for p in net.parameters():
            if not p.is_cuda or p.device != dev:
                raise ops.GanffnError("%s: every parameter must be on one GPU (got %s and %s); there is no CPU "
                                      "fallback" % (what, dev, p.device))

    def _init_positions(self, dev):
        self.device = dev
        self.positions = torch.zeros(self.capacity, device=dev, dtype=torch.int32)
        self._host_pos = [0] * self.capacity      # host mirror: only step, extend and reset change the positions
        self._bufs = {}
        self._ext_bufs = {}

    # ---- state ----------------------------------------------------------------------------------------------------
    def _check_slots(self, slots, what, n=None, unit=None):
        """a slot list (ints or an int tensor) as distinct ints in [0, capacity).  With n, a call's slot list for its n rows or
        columns (`unit`: what the message calls them), None meaning every slot -> a tuple of n"""
        if slots is None:
            if n != self.capacity:
                raise ValueError("%s: slots=None means every slot: n must be the capacity %d, got %d" % (what, self.capacity, n))
            slots = range(self.capacity)
        slots = [int(s) for s in (slots.tolist() if torch.is_tensor(slots) else slots)]
        for s in slots:
            if not 0 <= s < self.capacity:
                raise ValueError("%s: slot %d outside [0, %d)" % (what, s, self.capacity))
        if len(set(slots)) != len(slots):
            raise ValueError("%s: slots must be distinct, got %r" % (what, slots))
        if n is None:
            return slots
        if len(slots) != n or n < 1:
            raise ValueError("%s: %d %s for %d slots" % (what, n, unit, len(slots)))
        return tuple(slots)

    def reset(self, slots=None):
        """positions of the given slots (all by default) back to 0; the stale cache behind them is never read"""
        if slots is None:
            self.positions.zero_()
            self._host_pos = [0] * self.capacity
            return
        slots = self._check_slots(slots, "reset")
        if slots:
            self.positions.index_fill_(0, torch.tensor(slots, dtype=torch.int64, device=self.device), 0)
            for s in slots:
                self._host_pos[s] = 0

    def _check_not_full(self, slots, what):
        for s in slots:
            if self._host_pos[s] >= self.max_len:
                raise ValueError("%s: slot %d is full (%d utterances); reset() it before its next dialogue" % (what, s, self.max_len))

    def _check_lengths(self, m, n, lengths, slots, what):
        """an extend's m, its slot list and lengths -> (slots, lengths) as tuples; nothing launched"""
        if not 1 <= m <= self.max_len:
            raise ValueError("%s: m=%d utterances per call outside [1, max_len=%d]" % (what, m, self.max_len))
        slots = self._check_slots(slots, what, n, "columns")
        lengths = tuple(int(c) for c in (lengths.tolist() if torch.is_tensor(lengths) else lengths))
        if len(lengths) != n:
            raise ValueError("%s: %d lengths for %d columns" % (what, len(lengths), n))
        for s, c in zip(slots, lengths):
            if not 1 <= c <= m:
                raise ValueError("%s: length %d of slot %d outside [1, m=%d]" % (what, c, s, m))
        for s, c in zip(slots, lengths):
            if self._host_pos[s] + c > self.max_len:
                raise ValueError("%s: slot %d holds %d of max_len=%d utterances: %d more fit, not %d; reset() it before its next "
                                 "dialogue" % (what, s, self._host_pos[s], self.max_len, self.max_len - self._host_pos[s], c))
        return slots, lengths

    @staticmethod
    def _upload_slots(b, slots):
        if b.slots_host != slots:
            b.slot.copy_(torch.tensor(slots, dtype=torch.int32))
            b.slot64.copy_(b.slot)
            b.slots_host = slots

    @staticmethod
    def _upload_counts(b, lengths):
        if b.counts_host != lengths:
            b.count.copy_(torch.tensor(lengths, dtype=torch.int32))
            b.counts_host = lengths

    def _advance(self, b, count, slots, lengths):
        """the slots' positions += lengths (count: the same on the device), on the device and in the host mirror"""
        self.positions.index_add_(0, b.slot64, count)
        for s, c in zip(slots, lengths):
            self._host_pos[s] += c


class _GeneratorStream(_SlotStream):
    """What the generator-backed streaming sessions share besides the slots (_SlotStream): the three causal generators' per-layer
    K/V caches, stack configurations and workspaces, and the body of a step and of an extend up to the generators' stack outputs:
    a session is its __init__ and what it runs on those outputs."""

    def _init_generators(self, net, capacity, max_len, dev, what, parties=None):
        capacity, max_len = self._check_capacity(capacity, max_len)
        if parties is not None and not 1 <= int(parties) <= ops.DRNN_MAX_PARTIES:
            raise ValueError("parties=%r out of range [1, %d]" % (parties, ops.DRNN_MAX_PARTIES))
        self.net, self.capacity, self.max_len = net, capacity, max_len
        self.gens = [getattr(net, k) for k in GEN_NAMES]
        self._check_one_gpu(net, dev, what)
        self.cfgs, self.caches, self.ws, self.pes = [], [], [], []
        for g in self.gens:
            cfg = ops.enc_cfg(self.max_len, self.capacity, g.d_model, g.nhead, g.num_layers, train=False)
            n_cache, n_ws = ops.stream_sizes(cfg, self.capacity)
            self.cfgs.append(cfg)
            self.caches.append(torch.empty(n_cache, device=dev, dtype=torch.float32))     # never read at or above a position
            self.ws.append(torch.empty(n_ws, device=dev, dtype=torch.float32))
            self.pes.append(g.position_encoding.pe)
        self._init_positions(dev)

    def _heads_sum(self, b):
        """the generators' heads over the stack outputs b.enc and their sum -> b.fusion (returned)"""
        for i, g in enumerate(self.gens):
            ops.head_fwd_raw(b.head_cfg[i], b.enc[i], g.fc1.weight, g.fc1.bias, g.fc2.weight, g.fc2.bias, None, None,
                             b.head_out[i], b.head_saved[i], b.head_ws[i], None, 0)
        ops.add3_raw(b.head_out[0], b.head_out[1], b.head_out[2], b.fusion, b.fusion.numel())
        return b.fusion

    def _check_rows(self, xs, slots, what):
        """shapes of a step's inputs and its slot list -> (n, slots as a tuple); nothing full, nothing launched"""
        n = int(xs[0].shape[0])
        for x, g in zip(xs, self.gens):
            if x.dim() != 2 or x.shape[0] != n or x.shape[1] != g.d_model:
                raise ValueError("%s: inputs must be [n, 100], [n, 512], [n, 100]; got %s" % (what, [tuple(t.shape) for t in xs]))
        slots = self._check_slots(slots, what, n, "rows")
        self._check_not_full(slots, what)
        return n, slots

    def _check_chunks(self, xs, lengths, slots, what):
        """shapes of an extend's inputs, its slot list and lengths -> (m, n, slots, lengths as tuples); nothing launched"""
        if xs[0].dim() != 3:
            raise ValueError("%s: inputs must be [m, n, 100], [m, n, 512], [m, n, 100]; got %s" % (what, [tuple(t.shape) for t in xs]))
        m, n = int(xs[0].shape[0]), int(xs[0].shape[1])
        for x, g in zip(xs, self.gens):
            if x.dim() != 3 or x.shape[0] != m or x.shape[1] != n or x.shape[2] != g.d_model:
                raise ValueError("%s: inputs must be [m, n, 100], [m, n, 512], [m, n, 100]; got %s" % (what, [tuple(t.shape) for t in xs]))
        slots, lengths = self._check_lengths(m, n, lengths, slots, what)
        return m, n, slots, lengths

    def _new_bufs(self, m, n):
        """the buffers of a step over n rows (m None) or of an extend over [m, n]; a session with a head of its own adds its buffers"""
        return _Bufs(self, n) if m is None else _ExtBufs(self, m, n)

    def _prepare_step(self, xs, n, slots):
        """the buffers of a step at n (made on the first one), with this call's slots and inputs in them"""
        b = self._bufs.get(n)
        if b is None:
            b = self._bufs[n] = self._new_bufs(None, n)
        if b.slots_host != slots:
            self._upload_slots(b, slots)
        for dst, x in zip(b.x, xs):
            dst.copy_(x)
        return b

    def _generator_steps(self, b, n):
        """one stack step per generator over the n new rows b.x -> b.enc"""
        for i, g in enumerate(self.gens):
            ops.encoder_stream_step_raw(self.cfgs[i], n, b.slot, self.positions, b.x[i], self.pes[i], g.slab, self.caches[i],
                                        b.enc[i], self.ws[i])

    def _prepare_extend(self, m, n, slots, lengths):
        """the buffers of an extend at (m, n) (made on the first one), with this call's slots and lengths in them"""
        b = self._ext_bufs.get((m, n))
        if b is None:
            b = self._ext_bufs[(m, n)] = self._new_bufs(m, n)
        self._upload_slots(b, slots)
        self._upload_counts(b, lengths)
        return b

    def _extend_groups(self, b, xs, m, tail, out):
        """the generators' extend over each group of dialogues, then tail(r) on the group's row buffers r; what it returns
        ([m * ng, W]) is the group's columns of out [m, n, W] (one group: out is that buffer itself)"""
        single = len(b.groups) == 1
        for lo, hi in b.groups:
            ng = hi - lo
            r = b.rows[ng]
            for i, g in enumerate(self.gens):
                xg = r.x[i].view(m, ng, g.d_model)
                xg.copy_(xs[i] if single else xs[i][:, lo:hi])
                ops.encoder_stream_extend_raw(self.cfgs[i], ng, m, b.slot[lo:hi], b.count[lo:hi], self.positions, xg, self.pes[i],
                                              g.slab, self.caches[i], r.enc[i], b.ws[i])
            res = tail(r)
            if not single:
                out[:, lo:hi].copy_(res.view(m, ng, -1))


class StreamSession(_GeneratorStream):
    """Per-dialogue K/V caches of a causal GAN_FFN and the step that labels one new utterance of up to `capacity` concurrent
    dialogues.  Slot s holds one dialogue; `positions[s]` (device int32) is the number of its utterances seen so far.

    Always eval math under no_grad (no dropout), whatever net.training says; the weights are read from the generators' slabs at
    call time.  CHANGED WEIGHTS: after a training step (or load_state_dict) the cached K / V are stale — call reset() and `extend`
    with the dialogues' utterances so far (one causal pass over them instead of one step per utterance); the session does not
    notice.  mask_padding is irrelevant to a stream: at real utterances lengths add nothing
    to a causal mask."""

    def __init__(self, net, capacity=1, max_len=None, use_graph=False):
        if not getattr(net, "causal", False):
            raise ValueError("GAN_FFN.stream() needs a classifier built with causal=True: row t of a bidirectional classifier "
                             "depends on the utterances after it, so it cannot be labelled as it arrives")
        self.use_graph = bool(use_graph)
        self._init_generators(net, capacity, max_len, net.fc.weight.device, "GAN_FFN.stream()")

    def _fusion_width(self):
        return self.net.fc.weight.shape[1]

    # ---- one utterance per active dialogue ---------------------------------------------------------------------------
    def _body(self, b, n):
        """the launches of a step, on the current stream: one stack step and one head per generator, sum, fc, log_softmax,
        then the position advance"""
        self._generator_steps(b, n)
        self._tail(b)
        self.positions.index_add_(0, b.slot64, b.ones)

    def _tail(self, b):
        """the row-wise rest of the classifier over the rows of stack outputs b.enc: the generators' heads, sum, fc, log_softmax
        -> b.log_prob"""
        net, n = self.net, b.fusion.shape[0]
        self._heads_sum(b)
        ops.linear_fwd_raw(b.fusion, net.fc.weight, net.fc.bias, b.logits, n, net.fc.weight.shape[1], net.n_classes)
        ops.logsoftmax_nll_raw(b.logits, None, None, None, b.log_prob, None, None, None, 1, n, net.n_classes)
        return b.log_prob

    def _graph_key(self):
        """the addresses a captured graph froze: a re-packed slab (a .to() that moved the module) asks for a new capture"""
        return tuple(g.slab.data_ptr() for g in self.gens) + (self.net.fc.weight.data_ptr(), self.net.fc.bias.data_ptr())

    @torch.no_grad()
    def step(self, acoustic, visual, text, slots=None):
        """acoustic [n, 100], visual [n, 512], text [n, 100]: the next utterance of n dialogues -> log_prob [n, n_classes].
        slots: None = slots 0 .. capacity-1 (then n == capacity), or n distinct ints in [0, capacity) (list or int tensor):
        row i belongs to the dialogue in slot slots[i].  Raises ValueError, before any launch, for a slot that is full
        (max_len utterances).  Never reads from the device (pass slots as a list: an int tensor is brought to the host to be
        validated, which for a device tensor is a read); allocates only on the first step at a given n.  The returned tensor is
        the session's buffer for that n: the next step with the same n overwrites it."""
        xs = (acoustic, visual, text)
        n, slots = self._check_rows(xs, slots, "step")
        b = self._prepare_step(xs, n, slots)
        if not self.use_graph:
            self._body(b, n)
        else:
            key = self._graph_key()
            if b.graph is not None and b.graph_key == key:
                b.graph.replay()
            else:
                # the first step at this n runs eagerly (lazy initialisation happens here, and its results are the step's);
                # the capture that follows records the same launches without running them
                self._body(b, n)
                torch.cuda.synchronize()
                b.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(b.graph):
                    self._body(b, n)
                b.graph_key = key
        for s in slots:                     # (the device side of the advance: in _body, for the graph)
            self._host_pos[s] += 1
        return b.log_prob

    # ---- several utterances per active dialogue --------------------------------------------------------------------------
    @torch.no_grad()
    def extend(self, acoustic, visual, text, lengths, slots=None):
        """acoustic [m, n, 100], visual [m, n, 512], text [m, n, 100], time-major (a padded batch of dialogue pieces passes straight
        in): the next lengths[i] utterances (n host ints, 1 <= lengths[i] <= m) of n dialogues -> log_prob [m, n, n_classes].
        slots: as in `step`.  Labels all new utterances in one causal pass, appends their K / V in every layer of the three
        generators and advances the positions by `lengths`, on the device and in the host mirror.  Rows j >= lengths[i] of the
        inputs must be finite (they run through the row-wise kernels; their values change no bit of a valid row or of the caches)
        and the same rows of the result are unspecified.  Raises ValueError, before any launch and with no position moved, for wrong
        shapes, slots that repeat or lie outside the capacity, a length outside [1, m] and a dialogue that would pass max_len.
        Never reads from the device (pass lengths and slots as lists), allocates only on the first call at a given (m, n), always
        runs eagerly (no graph).  One native call carries at most ops.STREAM_EXTEND_MAX_ROWS rows; a larger [m, n] runs over groups
        of dialogues, which do not interact (the kernels' summation-order rules are evaluated for a group's rows, as a step's are
        for its n).  Values agree with `step` by `step` and with the full causal forward to rounding, not bit for bit.  The returned
        tensor is the session's buffer for that (m, n): the next extend at the same (m, n) overwrites it."""
        xs = (acoustic, visual, text)
        m, n, slots, lengths = self._check_chunks(xs, lengths, slots, "extend")
        b = self._prepare_extend(m, n, slots, lengths)
        self._extend_groups(b, xs, m, self._tail, b.log_prob)
        self._advance(b, b.count, slots, lengths)
        return b.log_prob


# ---- configuration 5: the causal DialogueRNN classifier ------------------------------------------------------------------------
class _HeadBufs:
    """what the streamed head of a call over `rows` rows (n of a step, m * n of an extend) touches besides the generators' buffers"""

    def __init__(self, sess, rows, spk_shape):
        um = sess.net.bi_model
        f32 = dict(device=sess.device, dtype=torch.float32)
        self.spk = torch.zeros(spk_shape, device=sess.device, dtype=torch.int32)
        self.spk_host = None
        self.e = torch.empty(rows, um.D_e, **f32)
        self.xt = torch.empty(rows, um.D_e, **f32)
        self.att = torch.empty(rows, um.D_e, **f32)
        self.hidden = torch.empty(rows, um.linear.weight.shape[0], **f32)
        self.logits = torch.empty(rows, sess.net.n_classes, **f32)
        self.log_prob = torch.empty(rows, sess.net.n_classes, **f32)

    def upload_speakers(self, spk):
        if self.spk_host != spk:
            self.spk.copy_(torch.tensor(spk, dtype=torch.int32).view(self.spk.shape))
            self.spk_host = spk


class DrnnStreamSession(_GeneratorStream):
    """The streaming form of GAN_FFN_DialogueRNN(causal=True): per-dialogue K/V caches of the three causal generators (as
    StreamSession keeps them) and, next to them, the head's per-slot state — the global history g_0 .. g_{t-1}, the party states and
    the emotion history e_0 .. e_{t-1}, which is also the memory of the second attention (csrc/drnn_stream.hip; layout in
    include/ganffn.h).  `step` runs ONE recurrence step per new utterance instead of the whole prefix: log_prob[t] of the causal
    classifier depends on utterances and speakers 0 .. t only, so each row is final when it is returned.

    Always eval math under no_grad (no dropout), whatever net.training says; the weights are read from the net's parameter tensors
    at call time.  CHANGED WEIGHTS: the caches and the state are stale after a training step — reset() and `extend` with the
    dialogues so far.  Values agree with the rows of the net's full causal forward to rounding, not bit for bit."""

    def __init__(self, net, capacity=1, max_len=None, parties=2):
        if not getattr(net, "causal", False):
            raise ValueError("GAN_FFN_DialogueRNN.stream() needs a classifier built with causal=True: the bidirectional head reads "
                             "the future (its reverse DialogueRNN starts at the dialogue's last utterance), so no row can be "
                             "labelled as it arrives")
        um = net.bi_model
        cell = um.dialog_rnn_f.dialogue_cell
        self._init_generators(net, capacity, max_len, um.linear.weight.device, "GAN_FFN_DialogueRNN.stream()", parties)
        self.parties = int(parties)
        att = ops.drnn_att_type(cell)
        if cell.D_g != cell.D_p:
            raise ValueError("stream(): the step kernels need D_g == D_p, got D_g=%d D_p=%d" % (cell.D_g, cell.D_p))
        if cell.D_g > 512:
            raise ValueError("stream(): D_g = D_p = %d > 512 (the step kernels hold one state column per thread)" % cell.D_g)
        if cell.D_m % 4 or cell.D_g % 4 or cell.D_e % 4 or cell.D_e > 1024:
            raise ValueError("stream(): D_m=%d, D_g=%d, D_e=%d must be multiples of 4, D_e <= 1024" % (cell.D_m, cell.D_g, cell.D_e))
        if att == "dot" and cell.D_m != cell.D_g:
            raise ValueError("stream(): dot attention needs D_m == D_g, got D_m=%d D_g=%d" % (cell.D_m, cell.D_g))
        Da = cell.attention.transform.weight.shape[0] if att == "concat" else 0
        if att == "concat" and (Da % 4 or not 4 <= Da <= 512):
            raise ValueError("stream(): concat attention needs D_a a multiple of 4 in [4, 512], got D_a=%d" % Da)
        for g in self.gens:
            if g.fc2.weight.shape[0] != cell.D_m:
                raise ValueError("stream(): the generators' output width %d is not D_m=%d" % (g.fc2.weight.shape[0], cell.D_m))
        self.cell, self.um = cell, um
        self.head_cfg = ops.drnn_stream_cfg(self.capacity, self.max_len, self.parties, cell.D_m, cell.D_g, cell.D_e,
                                            cell.listener_state, att, Da)
        n_state, n_ws = ops.drnn_stream_sizes(self.head_cfg, self.capacity)
        self.state = torch.empty(n_state, device=self.device, dtype=torch.float32)      # never read at or above a position
        self.head_ws = torch.empty(n_ws, device=self.device, dtype=torch.float32)
        a4 = lambda k: (k + 3) & ~3                                                     # noqa: E731  (the header's region rule)
        e_off = a4(self.capacity * self.max_len * cell.D_g) + a4(self.capacity * self.parties * cell.D_g)
        self.e_hist = self.state[e_off:e_off + self.capacity * self.max_len * cell.D_e]  # the E region: the second attention's memory

    def _fusion_width(self):
        return self.cell.D_m

    def _new_bufs(self, m, n):
        b = super()._new_bufs(m, n)
        b.head = _HeadBufs(self, (m or 1) * n, (n,) if m is None else (m, n))
        if m is not None:
            b.fusion = (b.rows[n].fusion.view(m, n, -1) if len(b.groups) == 1 else
                        torch.empty(m, n, self.cell.D_m, device=self.device, dtype=torch.float32))
        return b

    def _check_speakers(self, speakers, shape, lengths, what):
        """speakers as host ints of the given shape, validated against the party count (entries past a length: ignored, sent as 0)"""
        spk = speakers.tolist() if torch.is_tensor(speakers) else speakers
        if len(shape) == 1:
            spk = tuple(int(v) for v in spk)
            if len(spk) != shape[0]:
                raise ValueError("%s: %d speakers for %d rows" % (what, len(spk), shape[0]))
            live = spk
        else:
            m, n = shape
            if len(spk) != m or any(len(r) != n for r in spk):
                raise ValueError("%s: speakers must be [m=%d][n=%d] ints" % (what, m, n))
            spk = tuple(int(spk[j][i]) if j < lengths[i] else 0 for j in range(m) for i in range(n))
            live = spk
        for v in live:
            if not 0 <= v < self.parties:
                raise ValueError("%s: speaker %d outside [0, parties=%d)" % (what, v, self.parties))
        return spk

    def _head_tail(self, h, fusion, b, n, m, count):
        """the head over m * n time-major rows of fusion: recurrence (one step, or the native extend), transform, the second
        attention over the slot's emotion history, linear + ReLU, smax_fc, log_softmax"""
        um, rows = self.um, m * n
        De, Dh, Cn = um.D_e, um.linear.weight.shape[0], self.net.n_classes
        ptrs = ops.drnn_stream_cell_ptrs(self.cell)
        if count is None:
            ops.drnn_stream_step_raw(self.head_cfg, n, b.slot, self.positions, h.spk, fusion, ptrs, self.state, h.e, self.head_ws)
        else:
            ops.drnn_stream_extend_raw(self.head_cfg, n, m, b.slot, count, self.positions, h.spk, fusion, ptrs, self.state, h.e,
                                       self.head_ws)
        tr = um.matchatt.transform
        ops.linear_fwd_raw(h.e, tr.weight, tr.bias, h.xt, rows, De, De)
        ops.general2_stream_attention_raw(h.xt, self.e_hist, b.slot, count, self.positions, h.att, None, n, m, self.capacity,
                                          self.max_len, De)
        ops.linear1_fwd_raw(h.att, um.linear.weight, um.linear.bias, h.hidden, rows, De, Dh, 0.0, 0, None, 0, False)
        ops.linear_fwd_raw(h.hidden, um.smax_fc.weight, um.smax_fc.bias, h.logits, rows, Dh, Cn)
        ops.logsoftmax_nll_raw(h.logits, None, None, None, h.log_prob, None, None, None, 1, rows, Cn)

    # ---- one utterance per active dialogue ---------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, acoustic, visual, text, speakers, slots=None):
        """acoustic [n, 100], visual [n, 512], text [n, 100]: the next utterance of n dialogues; speakers: n host ints in
        [0, parties) (or an int tensor, which is brought to the host to be validated) — the party index, not a one-hot.
        -> log_prob [n, n_classes].  slots: as in StreamSession.step.  Everything — shapes, slots, a full slot, a speaker out of
        range — is validated before any launch and with no position moved.  Never reads from the device, allocates only on the
        first step at a given n; the returned tensor is the session's buffer for that n."""
        xs = (acoustic, visual, text)
        n, slots = self._check_rows(xs, slots, "step")
        spk = self._check_speakers(speakers, (n,), None, "step")
        b = self._prepare_step(xs, n, slots)
        b.head.upload_speakers(spk)
        self._generator_steps(b, n)
        self._heads_sum(b)
        self._head_tail(b.head, b.fusion, b, n, 1, None)
        self._advance(b, b.ones, slots, (1,) * n)
        return b.head.log_prob

    # ---- several utterances per active dialogue --------------------------------------------------------------------------
    @torch.no_grad()
    def extend(self, acoustic, visual, text, speakers, lengths, slots=None):
        """acoustic [m, n, 100], visual [m, n, 512], text [m, n, 100], time-major; speakers [m][n] host ints (entries at
        j >= lengths[i] are ignored); lengths: n host ints in [1, m] -> log_prob [m, n, n_classes], rows past a length unspecified.
        One generator extend per group of at most ops.STREAM_EXTEND_MAX_ROWS rows, then ONE native head extend (the recurrence is
        serial in t: lengths[i] steps per dialogue with no host synchronisation), then the row-wise tail.  Raises ValueError before
        any launch and with no position moved, as StreamSession.extend does, and for a speaker out of range.  Rows past a length
        must be finite."""
        xs = (acoustic, visual, text)
        m, n, slots, lengths = self._check_chunks(xs, lengths, slots, "extend")
        spk = self._check_speakers(speakers, (m, n), lengths, "extend")
        b = self._prepare_extend(m, n, slots, lengths)
        b.head.upload_speakers(spk)
        self._extend_groups(b, xs, m, self._heads_sum, b.fusion)
        self._head_tail(b.head, b.fusion, b, n, m, b.count)
        self._advance(b, b.count, slots, lengths)
        return b.head.log_prob.view(m, n, -1)


# ---- the causal MELD classifier -----------------------------------------------------------------------------------------------
class _MeldBufs:
    """everything a MELD step over n rows (m None) or an extend over [m, n] touches: allocated on the first call at that n or
    (m, n), never again"""

    def __init__(self, sess, m, n):
        dev, f32 = sess.device, dict(device=sess.device, dtype=torch.float32)
        rows, De, Cn = (m or 1) * n, sess.D_e, sess.model.n_classes
        self.slot = torch.zeros(n, device=dev, dtype=torch.int32)
        self.slot64 = torch.zeros(n, device=dev, dtype=torch.int64)
        self.ones = torch.ones(n, device=dev, dtype=torch.int32)
        self.count = torch.zeros(n, device=dev, dtype=torch.int32) if m is not None else None
        self.slots_host = self.counts_host = None                       # what the device copies hold, to skip equal uploads
        self.x = torch.zeros(rows, sess.D_m, **f32)
        self.e = torch.empty(rows, De, **f32)
        self.xt = torch.empty(rows, De, **f32)
        self.att = torch.empty(rows, De, **f32)
        self.hidden = torch.empty(rows, De, **f32)
        self.logits = torch.empty(rows, Cn, **f32)
        self.log_prob = torch.empty(rows, Cn, **f32)


class MeldStreamSession(_SlotStream):
    """The streaming form of MELDLSTMModel(causal=True): per slot, (h, c) of every LSTM layer after the dialogue's last utterance
    and the emotion history e_0 .. e_{t-1}, which is the memory of the causal general2 attention (csrc/lstm_stream.hip; layout in
    include/ganffn.h).  `step` runs ONE LSTM step per new utterance instead of the whole prefix: log_prob[t] of the causal
    classifier depends on utterances 0 .. t only, so each row is final when it is returned.  A step is 13 launches of the library
    at four layers: the LSTM step's 9, then matchatt.transform, the single-query general2 attention over the slot's history,
    hardswish(e + hardswish(att)) with smax_fc, log_softmax.

    Always eval math under no_grad (no dropout), whatever model.training says; the weights are read from the model's parameter
    tensors at call time.  CHANGED WEIGHTS: the state is stale after a training step — reset() and `extend` with the dialogues so
    far.  `packed` is irrelevant to a stream, which has no padding.  Values agree with the rows of the model's full causal
    forward to rounding, not bit for bit."""

    def __init__(self, model, capacity=1, max_len=None):
        if not getattr(model, "causal", False):
            raise ValueError("MELDLSTMModel.stream() needs a classifier built with causal=True: the bidirectional LSTM reads the "
                             "future (its reverse direction starts at the dialogue's end), so no row can be labelled as it arrives")
        lstm = model.lstm
        if model.D_h != model.D_e:
            raise ValueError("MELDLSTMModel.stream(): the att2=True branch hands the D_e-wide hidden to smax_fc, so it needs "
                             "D_h == D_e; got D_e=%d D_h=%d" % (model.D_e, model.D_h))
        if lstm.bidirectional or not ops.lstm_supported(lstm):
            raise ValueError("MELDLSTMModel.stream(): the LSTM must be forward-only with the layout ops.lstm_supported accepts "
                             "((seq, batch, feature), biases, no projection, input and hidden sizes multiples of 4)")
        if lstm.hidden_size > ops.LSTM_STREAM_MAX_H or not 1 <= lstm.num_layers <= ops.LSTM_STREAM_MAX_LAYERS:
            raise ValueError("MELDLSTMModel.stream(): D_e=%d, num_layers=%d outside the step kernels' limits (D_e <= %d, 1 .. %d "
                             "layers)" % (lstm.hidden_size, lstm.num_layers, ops.LSTM_STREAM_MAX_H, ops.LSTM_STREAM_MAX_LAYERS))
        if not 1 <= model.n_classes <= ops.MELD_HEAD_MAX_CLASSES:
            raise ValueError("MELDLSTMModel.stream(): n_classes=%d outside [1, %d]" % (model.n_classes, ops.MELD_HEAD_MAX_CLASSES))
        self.capacity, self.max_len = self._check_capacity(capacity, max_len)
        self.model, self.lstm = model, lstm
        self.D_m, self.D_e, self.L = lstm.input_size, lstm.hidden_size, lstm.num_layers
        dev = model.smax_fc.weight.device
        self._check_one_gpu(model, dev, "MELDLSTMModel.stream()")
        self.cfg = ops.lstm_stream_cfg(self.capacity, self.max_len, self.D_m, self.D_e, self.L)
        n_state, n_ws = ops.lstm_stream_sizes(self.cfg, self.capacity)
        self.state = torch.empty(n_state, device=dev, dtype=torch.float32)            # never read at or above a position
        self.ws = torch.empty(n_ws, device=dev, dtype=torch.float32)
        a4 = lambda k: (k + 3) & ~3                                                   # noqa: E731  (the header's region rule)
        e_off = 2 * a4(self.capacity * self.L * self.D_e)
        self.e_hist = self.state[e_off:e_off + self.capacity * self.max_len * self.D_e]  # the E region: the attention's memory
        self._init_positions(dev)

    def _buffers(self, m, n):
        cache, key = (self._bufs, n) if m is None else (self._ext_bufs, (m, n))
        b = cache.get(key)
        if b is None:
            b = cache[key] = _MeldBufs(self, m, n)
        return b

    def _run(self, b, n, m, count):
        """the launches of a call over m * n time-major rows b.x: the LSTM (one step, or the native extend), transform, the
        attention over the slot's emotion history, the hardswish head with smax_fc, log_softmax -> b.log_prob"""
        mod, rows, De, Cn = self.model, m * n, self.D_e, self.model.n_classes
        ptrs = ops.lstm_stream_ptrs(self.lstm)                 # (refuses parameters that left the GPU: before any launch)
        if count is None:
            ops.lstm_stream_step_raw(self.cfg, n, b.slot, self.positions, b.x, ptrs, self.state, b.e, self.ws)
        else:
            ops.lstm_stream_extend_raw(self.cfg, n, m, b.slot, count, self.positions, b.x, ptrs, self.state, b.e, self.ws)
        tr = mod.matchatt.transform
        ops.linear_fwd_raw(b.e, tr.weight, tr.bias, b.xt, rows, De, De)
        ops.general2_stream_attention_raw(b.xt, self.e_hist, b.slot, count, self.positions, b.att, None, n, m, self.capacity,
                                          self.max_len, De)
        ops.meld_head_fwd_raw(b.e, b.att, mod.smax_fc.weight, mod.smax_fc.bias, b.hidden, b.logits, rows, De, Cn)
        ops.logsoftmax_nll_raw(b.logits, None, None, None, b.log_prob, None, None, None, 1, rows, Cn)

    # ---- one utterance per active dialogue ---------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, text, slots=None):
        """text [n, D_m]: the next utterance of n dialogues -> log_prob [n, n_classes].  slots: None = slots 0 .. capacity-1 (then
        n == capacity), or n distinct ints in [0, capacity) (list or int tensor): row i belongs to the dialogue in slot slots[i].
        Everything — the shape, the slots, a full slot (max_len utterances) — is validated before any launch and with no position
        moved (ValueError).  Never reads from the device (pass slots as a list), allocates only on the first step at a given n;
        the returned tensor is the session's buffer for that n: the next step with the same n overwrites it."""
        if text.dim() != 2 or text.shape[1] != self.D_m:
            raise ValueError("step: text must be [n, %d]; got %s" % (self.D_m, tuple(text.shape)))
        n = int(text.shape[0])
        slots = self._check_slots(slots, "step", n, "rows")
        self._check_not_full(slots, "step")
        b = self._buffers(None, n)
        self._upload_slots(b, slots)
        b.x.copy_(text)
        self._run(b, n, 1, None)
        self._advance(b, b.ones, slots, (1,) * n)
        return b.log_prob

    # ---- several utterances per active dialogue --------------------------------------------------------------------------
    @torch.no_grad()
    def extend(self, text, lengths, slots=None):
        """text [m, n, D_m], time-major (a padded batch of dialogue pieces passes straight in): the next lengths[i] utterances
        (n host ints, 1 <= lengths[i] <= m) of n dialogues -> log_prob [m, n, n_classes], rows past a length unspecified.  ONE
        native LSTM extend (the recurrence is serial in t: lengths[i] steps per dialogue with no host synchronisation), then the
        row-wise tail over all rows; the positions advance by `lengths`, on the device and in the host mirror.  Rows j >=
        lengths[i] of text must be finite; their values change no bit of a valid row or of the state.  Raises ValueError before
        any launch and with no position moved for a wrong shape, slots that repeat or lie outside the capacity, a length outside
        [1, m] and a dialogue that would pass max_len.  Never reads from the device, allocates only on the first call at a given
        (m, n); the returned tensor is the session's buffer for that (m, n)."""
        if text.dim() != 3 or text.shape[2] != self.D_m:
            raise ValueError("extend: text must be [m, n, %d]; got %s" % (self.D_m, tuple(text.shape)))
        m, n = int(text.shape[0]), int(text.shape[1])
        slots, lengths = self._check_lengths(m, n, lengths, slots, "extend")
        b = self._buffers(m, n)
        self._upload_slots(b, slots)
        self._upload_counts(b, lengths)
        b.x.view(m, n, self.D_m).copy_(text)
        self._run(b, n, m, b.count)
        self._advance(b, b.count, slots, lengths)
        return b.log_prob.view(m, n, -1)
