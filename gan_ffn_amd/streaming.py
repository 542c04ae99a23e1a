"""Streaming causal classifier: label each utterance as it arrives.

`GAN_FFN(causal=True).stream(capacity, max_len)` returns a StreamSession.  Under the causal mask the K and V of a past utterance
never change and everything else in the classifier is row-wise (positional encoding, LayerNorm, FFN, the GELU head, the sum, `fc`,
log_softmax), so `step` runs the three generators on the NEW rows alone against per-layer K/V caches (csrc/stream.hip,
ganffn_encoder_stream_step) instead of on the whole prefix: constant rows and constant memory traffic per utterance.  A step's
values agree with the matching rows of the full causal forward to rounding, not bit for bit (the kernels' summation-order
rules are evaluated for n rows).  `extend` ingests several utterances per dialogue in one call (ganffn_encoder_stream_extend: one
causal pass over the new rows against the same caches) — a dialogue joined under way, caches rebuilt after the weights changed,
utterances that arrive in bursts.
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
        self.fusion = torch.empty(n, sess.net.fc.weight.shape[1], **f32)
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


class StreamSession:
    """Per-dialogue K/V caches of a causal GAN_FFN and the step that labels one new utterance of up to `capacity` concurrent
    dialogues.  Slot s holds one dialogue; `positions[s]` (device int32) is the number of its utterances seen so far.

    Always eval math under no_grad (no dropout), whatever net.training says; the weights are read from the generators' slabs at
    call time.  CHANGED WEIGHTS: after a training step (or load_state_dict) the cached K / V are stale — call reset() and `extend`
    with the dialogues' utterances so far (one causal pass over them instead of one step per utterance); the session does not
    notice.  mask_padding is irrelevant to a stream: at real utterances lengths add nothing
    to a causal mask."""

    def __init__(self, net, capacity=1, max_len=None, use_graph=False):
        from .model import MAX_LEN
        max_len = MAX_LEN if max_len is None else int(max_len)
        if not getattr(net, "causal", False):
            raise ValueError("GAN_FFN.stream() needs a classifier built with causal=True: row t of a bidirectional classifier "
                             "depends on the utterances after it, so it cannot be labelled as it arrives")
        if not 1 <= int(capacity) <= MAX_DIALOGUES:
            raise ValueError("capacity=%r out of range [1, %d]" % (capacity, MAX_DIALOGUES))
        if not 1 <= max_len <= MAX_LEN:
            raise ValueError("max_len=%r out of range [1, %d] (PositionalEncoding max_len)" % (max_len, MAX_LEN))
        self.net, self.capacity, self.max_len, self.use_graph = net, int(capacity), max_len, bool(use_graph)
        self.gens = [getattr(net, k) for k in GEN_NAMES]
        dev = net.fc.weight.device
        for p in net.parameters():
            if not p.is_cuda or p.device != dev:
                raise ops.GanffnError("GAN_FFN.stream(): every parameter must be on one GPU (got %s and %s); there is no CPU "
                                      "fallback" % (dev, p.device))
        self.device = dev
        self.cfgs, self.caches, self.ws, self.pes = [], [], [], []
        for g in self.gens:
            cfg = ops.enc_cfg(self.max_len, self.capacity, g.d_model, g.nhead, g.num_layers, train=False)
            n_cache, n_ws = ops.stream_sizes(cfg, self.capacity)
            self.cfgs.append(cfg)
            self.caches.append(torch.empty(n_cache, device=dev, dtype=torch.float32))     # never read at or above a position
            self.ws.append(torch.empty(n_ws, device=dev, dtype=torch.float32))
            self.pes.append(g.position_encoding.pe)
        self.positions = torch.zeros(self.capacity, device=dev, dtype=torch.int32)
        self._host_pos = [0] * self.capacity      # host mirror: only step, extend and reset change the positions
        self._bufs = {}
        self._ext_bufs = {}

    # ---- state ----------------------------------------------------------------------------------------------------
    def _check_slots(self, slots, what):
        slots = [int(s) for s in slots]
        for s in slots:
            if not 0 <= s < self.capacity:
                raise ValueError("%s: slot %d outside [0, %d)" % (what, s, self.capacity))
        if len(set(slots)) != len(slots):
            raise ValueError("%s: slots must be distinct, got %r" % (what, slots))
        return slots

    def reset(self, slots=None):
        """positions of the given slots (all by default) back to 0; the stale cache behind them is never read"""
        if slots is None:
            self.positions.zero_()
            self._host_pos = [0] * self.capacity
            return
        slots = self._check_slots(slots.tolist() if torch.is_tensor(slots) else slots, "reset")
        if slots:
            self.positions.index_fill_(0, torch.tensor(slots, dtype=torch.int64, device=self.device), 0)
            for s in slots:
                self._host_pos[s] = 0

    # ---- one utterance per active dialogue ---------------------------------------------------------------------------
    def _body(self, b, n):
        """the launches of a step, on the current stream: one stack step and one head per generator, sum, fc, log_softmax,
        then the position advance"""
        for i, g in enumerate(self.gens):
            ops.encoder_stream_step_raw(self.cfgs[i], n, b.slot, self.positions, b.x[i], self.pes[i], g.slab, self.caches[i],
                                        b.enc[i], self.ws[i])
        self._tail(b, n)
        self.positions.index_add_(0, b.slot64, b.ones)

    def _tail(self, b, n):
        """the row-wise rest of the classifier over n rows of stack outputs b.enc: the generators' heads, sum, fc, log_softmax"""
        net = self.net
        for i, g in enumerate(self.gens):
            ops.head_fwd_raw(b.head_cfg[i], b.enc[i], g.fc1.weight, g.fc1.bias, g.fc2.weight, g.fc2.bias, None, None,
                             b.head_out[i], b.head_saved[i], b.head_ws[i], None, 0)
        ops._lib.call("ganffn_add3", ops._ptr(b.head_out[0]), ops._ptr(b.head_out[1]), ops._ptr(b.head_out[2]), ops._ptr(b.fusion),
                      ops.C.c_int64(b.fusion.numel()), ops._stream())
        ops.linear_fwd_raw(b.fusion, net.fc.weight, net.fc.bias, b.logits, n, net.fc.weight.shape[1], net.n_classes)
        ops.logsoftmax_nll_raw(b.logits, None, None, None, b.log_prob, None, None, None, 1, n, net.n_classes)

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
        n = int(acoustic.shape[0])
        for x, g in zip(xs, self.gens):
            if x.dim() != 2 or x.shape[0] != n or x.shape[1] != g.d_model:
                raise ValueError("step: inputs must be [n, 100], [n, 512], [n, 100]; got %s" % [tuple(t.shape) for t in xs])
        if slots is None:
            if n != self.capacity:
                raise ValueError("step: slots=None means every slot: n must be the capacity %d, got %d" % (self.capacity, n))
            slots = range(self.capacity)
        slots = tuple(self._check_slots(slots.tolist() if torch.is_tensor(slots) else slots, "step"))
        if len(slots) != n or n < 1:
            raise ValueError("step: %d rows for %d slots" % (n, len(slots)))
        for s in slots:
            if self._host_pos[s] >= self.max_len:
                raise ValueError("step: slot %d is full (%d utterances); reset() it before its next dialogue" % (s, self.max_len))
        b = self._bufs.get(n)
        if b is None:
            b = self._bufs[n] = _Bufs(self, n)
        if b.slots_host != slots:
            b.slot.copy_(torch.tensor(slots, dtype=torch.int32))
            b.slot64.copy_(b.slot)
            b.slots_host = slots
        for dst, x in zip(b.x, xs):
            dst.copy_(x)
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
        for s in slots:
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
        if acoustic.dim() != 3:
            raise ValueError("extend: inputs must be [m, n, 100], [m, n, 512], [m, n, 100]; got %s" % [tuple(t.shape) for t in xs])
        m, n = int(acoustic.shape[0]), int(acoustic.shape[1])
        for x, g in zip(xs, self.gens):
            if x.dim() != 3 or x.shape[0] != m or x.shape[1] != n or x.shape[2] != g.d_model:
                raise ValueError("extend: inputs must be [m, n, 100], [m, n, 512], [m, n, 100]; got %s" % [tuple(t.shape) for t in xs])
        if not 1 <= m <= self.max_len:
            raise ValueError("extend: m=%d utterances per call outside [1, max_len=%d]" % (m, self.max_len))
        if slots is None:
            if n != self.capacity:
                raise ValueError("extend: slots=None means every slot: n must be the capacity %d, got %d" % (self.capacity, n))
            slots = range(self.capacity)
        slots = tuple(self._check_slots(slots.tolist() if torch.is_tensor(slots) else slots, "extend"))
        if len(slots) != n or n < 1:
            raise ValueError("extend: %d columns for %d slots" % (n, len(slots)))
        lengths = tuple(int(c) for c in (lengths.tolist() if torch.is_tensor(lengths) else lengths))
        if len(lengths) != n:
            raise ValueError("extend: %d lengths for %d columns" % (len(lengths), n))
        for s, c in zip(slots, lengths):
            if not 1 <= c <= m:
                raise ValueError("extend: length %d of slot %d outside [1, m=%d]" % (c, s, m))
        for s, c in zip(slots, lengths):
            if self._host_pos[s] + c > self.max_len:
                raise ValueError("extend: slot %d holds %d of max_len=%d utterances: %d more fit, not %d; reset() it before its next "
                                 "dialogue" % (s, self._host_pos[s], self.max_len, self.max_len - self._host_pos[s], c))
        b = self._ext_bufs.get((m, n))
        if b is None:
            b = self._ext_bufs[(m, n)] = _ExtBufs(self, m, n)
        if b.slots_host != slots:
            b.slot.copy_(torch.tensor(slots, dtype=torch.int32))
            b.slot64.copy_(b.slot)
            b.slots_host = slots
        if b.counts_host != lengths:
            b.count.copy_(torch.tensor(lengths, dtype=torch.int32))
            b.counts_host = lengths
        single = len(b.groups) == 1
        for lo, hi in b.groups:
            ng = hi - lo
            r = b.rows[ng]
            for i, g in enumerate(self.gens):
                xg = r.x[i].view(m, ng, g.d_model)
                xg.copy_(xs[i] if single else xs[i][:, lo:hi])
                ops.encoder_stream_extend_raw(self.cfgs[i], ng, m, b.slot[lo:hi], b.count[lo:hi], self.positions, xg, self.pes[i],
                                              g.slab, self.caches[i], r.enc[i], b.ws[i])
            self._tail(r, m * ng)
            if not single:
                b.log_prob[:, lo:hi].copy_(r.log_prob.view(m, ng, -1))
        self.positions.index_add_(0, b.slot64, b.count)
        for s, c in zip(slots, lengths):
            self._host_pos[s] += c
        return b.log_prob
