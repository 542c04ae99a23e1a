"""Streaming causal classifier: label each utterance as it arrives.

`GAN_FFN(causal=True).stream(capacity, max_len)` returns a StreamSession.  Under the causal mask the K and V of a past utterance
never change and everything else in the classifier is row-wise (positional encoding, LayerNorm, FFN, the GELU head, the sum, `fc`,
log_softmax), so `step` runs the three generators on the NEW rows alone against per-layer K/V caches (csrc/stream.hip,
ganffn_encoder_stream_step) instead of on the whole prefix: constant rows and constant memory traffic per utterance.  A step's
values agree with the matching rows of the full causal forward to rounding, not bit for bit (the kernels' summation-order
rules are evaluated for n rows).
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


class StreamSession:
    """Per-dialogue K/V caches of a causal GAN_FFN and the step that labels one new utterance of up to `capacity` concurrent
    dialogues.  Slot s holds one dialogue; `positions[s]` (device int32) is the number of its utterances seen so far.

    Always eval math under no_grad (no dropout), whatever net.training says; the weights are read from the generators' slabs at
    call time.  CHANGED WEIGHTS: after a training step (or load_state_dict) the cached K / V are stale — call reset() and step the
    dialogues again; the session does not notice.  mask_padding is irrelevant to a stream: at real utterances lengths add nothing
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
        self._host_pos = [0] * self.capacity      # host mirror: only step and reset change the positions
        self._bufs = {}

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
        net = self.net
        for i, g in enumerate(self.gens):
            ops.encoder_stream_step_raw(self.cfgs[i], n, b.slot, self.positions, b.x[i], self.pes[i], g.slab, self.caches[i],
                                        b.enc[i], self.ws[i])
            ops.head_fwd_raw(b.head_cfg[i], b.enc[i], g.fc1.weight, g.fc1.bias, g.fc2.weight, g.fc2.bias, None, None,
                             b.head_out[i], b.head_saved[i], b.head_ws[i], None, 0)
        ops._lib.call("ganffn_add3", ops._ptr(b.head_out[0]), ops._ptr(b.head_out[1]), ops._ptr(b.head_out[2]), ops._ptr(b.fusion),
                      ops.C.c_int64(b.fusion.numel()), ops._stream())
        ops.linear_fwd_raw(b.fusion, net.fc.weight, net.fc.bias, b.logits, n, net.fc.weight.shape[1], net.n_classes)
        ops.logsoftmax_nll_raw(b.logits, None, None, None, b.log_prob, None, None, None, 1, n, net.n_classes)
        self.positions.index_add_(0, b.slot64, b.ones)

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
