"""Fast step runner: the counterpart of the reference's train_disc / train_gen / train_GAN
(/root/reference/train_IEMOCAP.py:200-393), driving libganffn.so directly.

Differences from running the nn.Module mirror under torch autograd — all result-preserving:
  * no autograd graph: forward/backward are explicit C-ABI calls on preallocated buffers;
  * train_disc evaluates D(real) and D(fake) as ONE pass over a [real | fake] batch of 2B dialogues
    (dialogues are independent in every op; loss = ganffn_bce2 = (BCE(real,1)+BCE(fake,0))/2);
  * the generator forward inside train_disc keeps nothing for backward (the reference builds and
    discards that graph, train_IEMOCAP.py:218-219);
  * train_gen skips the frozen discriminator's weight gradients (computed but never used by the
    reference: zero_grad at train_IEMOCAP.py:216 clears them before D's next step);
  * losses stay on the device; the host reads all 12 once per iteration instead of 12 syncs
    (train_IEMOCAP.py:224,249);
  * gradients, Adam moments and parameters are flat slabs -> one fused Adam launch and, with
    world_size > 1, a bucketed all-reduce (RCCL) per sub-step;
  * optionally the whole iteration is captured once into a hipGraph and replayed (launch-bound otherwise).
"""
import ctypes as C
import os

import torch

from . import _lib, ops
from ._lib import HeadCfg

# sub-step schedule of one batch, train_IEMOCAP.py:355-382: (kind, trained net, partner net)
SCHEDULE = [
    ("D", "visual", "acoustic"), ("G", "acoustic", "visual"),
    ("D", "visual", "text"), ("G", "text", "visual"),
    ("D", "text", "acoustic"), ("G", "acoustic", "text"),
    ("D", "acoustic", "text"), ("G", "text", "acoustic"),
    ("D", "text", "visual"), ("G", "visual", "text"),
    ("D", "acoustic", "visual"), ("G", "visual", "acoustic"),
]
LOSS_COLUMNS = ["acoustic_G_loss", "visual_G_loss", "text_G_loss", "visual_D_loss", "text_D_loss",
                "acoustic_D_loss"]  # train_IEMOCAP.py:308-316


class NetState:
    """One network on the device: parameter slab (shared with the nn.Module), gradient slab, Adam state."""

    def __init__(self, module, lr, betas, weight_decay=0.0):
        self.m = module
        self.slab = module.slab
        assert self.slab.is_cuda, "NetState needs the module on the GPU"
        total, views, enc = module.slab_layout()
        self.total, self.views, self.enc_floats = total, views, enc
        self.grad = torch.zeros_like(self.slab)
        self.exp_avg = torch.zeros_like(self.slab)
        self.exp_avg_sq = torch.zeros_like(self.slab)
        self.step = torch.zeros(1, dtype=torch.int32, device=self.slab.device)
        self.lr, self.betas, self.wd = lr, betas, weight_decay
        self.E, self.H, self.L = module.d_model, module.nhead, module.num_layers
        self.kind = 0 if module.KIND == "gen" else 1
        named = {}
        params = module._slab_params()
        names = {id(p): n for n, p in module.named_parameters()}
        for p, (off, shape) in zip(params, views):
            named[names[id(p)]] = (off, shape)
        self.named = named
        self.pe = module.position_encoding.pe
        self.p_head = float(module.dropout.p)
        self.p_pe = float(module.position_encoding.dropout.p)
        self.p_enc = float(module.transformer_encoder.enc_dropout)
        self.D1 = module.fc1.weight.shape[0]
        self.D2 = module.fc2.weight.shape[0]
        self.layer_floats = enc // self.L
        self.covered = int(_lib.load().ganffn_encoder_bwd_parts_covered(self.E, 2048))    # chunked head of a layer block (weights, biases)
        self.has_obj = bool(module.HAS_OBJECT)
        self.obj_in = int(module.OBJECT_IN) if self.has_obj else 0       # raw-modality width `object` maps to D_h
        # `object` (weight [D_h x obj_in] | bias [D_h], each padded to 4 floats) sits right after the layers
        self.obj_floats = sum((int(p.numel()) + 3) & ~3 for p in (module.object.weight, module.object.bias)) if self.has_obj else 0

    def w(self, name, grad=False):
        off, shape = self.named[name]
        n = 1
        for d in shape:
            n *= d
        return (self.grad if grad else self.slab)[off:off + n]

    def buckets(self, n_buckets):
        """[(lo, hi)] float ranges of the grad slab, in the order backward completes them:
        head (+object) first, then encoder layers from the last to the first."""
        return bucket_ranges(self.enc_floats, self.obj_floats, self.total, self.layer_floats, self.L, n_buckets)


class _ParamSlab:
    """Module parameters that belong to no generator (a classifier head, an LSTM) packed into one slab: every tensor starts
    on a multiple of 4 floats, the parameters become views of the slab, and gradient, Adam moments and step count sit
    beside it — what NetState is for a generator."""

    def __init__(self, params, device):
        self.params = list(params)
        self.offs, total = [], 0
        for p_ in self.params:
            self.offs.append(total)
            total += (p_.numel() + 3) & ~3
        self.total = total
        self.slab = torch.zeros(total, device=device)
        with torch.no_grad():
            for i, p_ in enumerate(self.params):
                self.view(i).copy_(p_.detach().reshape(-1))
                p_.data = self.view(i).view_as(p_)
        self.grad = torch.zeros_like(self.slab)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.slab), torch.zeros_like(self.slab)
        self.step = torch.zeros(1, dtype=torch.int32, device=device)

    def view(self, i, grad=False):
        o, n = self.offs[i], self.params[i].numel()
        return (self.grad if grad else self.slab)[o:o + n]

    def in_place(self):
        """every parameter is still the view at its offset (a .to() / flatten_parameters since then gave it new storage, and
        the engine would silently stop following)"""
        base = self.slab.data_ptr()
        return all(p_.data_ptr() == base + 4 * o for p_, o in zip(self.params, self.offs))

    def all_reduce(self, pg, wait=True):
        """sum the gradient slab over the ranks of pg (None: nothing to do): in-line on the current stream (dp_mode()), or
        through a GradReducer — wait=False returns it unfinished, for the caller to finish() after more work is enqueued"""
        if pg is None:
            return None
        if dp_mode() == "inline":
            import torch.distributed as dist
            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=pg, async_op=False)
            return None
        red = GradReducer(pg)
        red.reduce_async(self.grad)
        if not wait:
            return red
        red.finish()
        return None

    def adam(self, lr, wd, world):
        ops.adam_step_raw(self.slab, self.grad, self.exp_avg, self.exp_avg_sq, self.step, self.total, lr, 0.9, 0.999, 1e-8,
                          wd, 1.0 / world)


def predictions(log_prob):
    """argmax over classes in the reference's batch-major flattening (train_IEMOCAP.py:154,158; train_MELD.py:72,76)"""
    return log_prob.transpose(0, 1).reshape(-1, log_prob.shape[2]).argmax(1)


def dp_mode():
    """how gradients cross the ranks (GANFFN_DP_MODE):
    "inline" (default, round 4): ONE all-reduce of the network's whole gradient slab per sub-step, issued as a synchronous
        collective — torch >= 2.7 runs those on the CURRENT stream, i.e. in-line on the sub-step's own HIP stream, between its
        backward and its Adam: no internal communication stream, no cross-stream events; the all-reduce of one sub-step runs
        beside the compute of the sub-steps on the other streams (each stream has its own communicator, so collectives of
        different streams never share one);
    "buckets" (rounds 1-3): 4-5 asynchronous all-reduces per sub-step on the process group's internal stream, each issued
        right after its layer range's backward, Adam per bucket.  Measured with a 1-rank RCCL group on one MI355X
        (tools/dist1_ab.sh): 40.6-60.6 ms per step against 34.5 ms for the plain engine — the internal stream's event waits
        share hardware queues with the sub-step streams and hold them up; see DESIGN.md section 7."""
    return os.environ.get("GANFFN_DP_MODE", "inline")


class GradReducer:
    """Bucketed gradient all-reduce for data parallelism over the DIALOGUE axis (one process per GPU).
    Each call sums one contiguous slice of a gradient slab across ranks, asynchronously (on RCCL's own
    stream for the nccl backend), so it overlaps whatever backward work is enqueued next; finish()
    makes the current stream wait for all of them.  The 1/world factor is applied by Adam (grad_scale).
    Backend-agnostic (nccl on MI355X, gloo in the CPU tests)."""

    def __init__(self, process_group):
        import torch.distributed as dist
        self.dist, self.pg = dist, process_group
        self.world = dist.get_world_size(process_group)
        self.works = []

    def reduce_async(self, flat_slice, lo=None, hi=None):
        w = self.dist.all_reduce(flat_slice, op=self.dist.ReduceOp.SUM, group=self.pg, async_op=True)
        self.works.append((w, lo, hi))

    def finish(self, on_bucket=None):
        """wait for the buckets in issue order; on_bucket(lo, hi) runs right after a bucket's all-reduce has been waited
        for (the engine applies Adam to that slice there, so only the LAST bucket's reduce is exposed)"""
        for w, lo, hi in self.works:
            w.wait()
            if on_bucket is not None and lo is not None:
                on_bucket(lo, hi)
        self.works = []


def bucket_ranges(enc_floats, obj_floats, total, layer_floats, L, n_buckets):
    """[(lo, hi)] float ranges of a gradient slab in the order backward completes them: fc head first,
    then groups of encoder layers from the last layer to the first (`object`, whose gradient is produced
    last, is reduced separately by the caller)."""
    out = [(enc_floats + obj_floats, total)]
    per = max(1, (L + n_buckets - 1) // max(1, n_buckets))
    hi = L
    while hi > 0:
        lo = max(0, hi - per)
        out.append((lo * layer_floats, hi * layer_floats))
        hi = lo
    return out


class _Pass:
    """Buffers of one forward(+backward) pass of one network for up to `B` dialogues of up to `S` steps.  Storage is
    flat and sized for that capacity; `resize(S, B)` re-derives the configs and the shaped views for a smaller batch
    without touching the allocator (real loaders deliver a different S every iteration and a short last batch)."""

    def __init__(self, net, S, B, dev, need_bwd, S_cap=None):
        self.net, self.B, self.dev, self.need_bwd = net, B, dev, need_bwd
        self.S_cap = max(S, S_cap or 0)
        self.B_cap = B
        E = net.E
        cfg = ops.enc_cfg(self.S_cap, B, E, net.H, net.L, train=True, p_pe=net.p_pe, p_enc=net.p_enc)
        n_saved, n_ws = ops.enc_sizes(cfg)
        h_saved, h_ws = ops.head_sizes(HeadCfg(self.S_cap * B, E, net.D1, net.D2, net.kind, net.p_head, 1))
        f32 = dict(device=dev, dtype=torch.float32)
        Tc = self.S_cap * B
        self._enc_out = torch.empty(Tc * E, **f32)
        self._saved = torch.empty(n_saved, **f32) if need_bwd else None
        self._hsaved = torch.empty(h_saved, **f32)
        self._out = torch.empty(Tc * (net.D2 if net.kind == 0 else 1), **f32)
        self._dx = torch.empty(Tc * E, **f32) if need_bwd else None
        self.n_ws = max(n_ws, h_ws)          # at capacity: workspace needs grow with S
        if ops.encoder_fwd_pair_supported(cfg):
            self.n_ws = max(self.n_ws, ops.encoder_fwd_pair_workspace_floats(cfg))
        self.resize(S)

    def resize(self, S, B=None):
        B = self.B_cap if B is None else B
        assert S <= self.S_cap and B <= self.B_cap
        net = self.net
        self.B = B
        E = net.E
        self.S, self.T = S, S * B
        self.cfg_train = ops.enc_cfg(S, B, E, net.H, net.L, train=True, p_pe=net.p_pe, p_enc=net.p_enc)
        self.cfg_eval = ops.enc_cfg(S, B, E, net.H, net.L, train=False, p_pe=net.p_pe, p_enc=net.p_enc)
        self.pair_ok = ops.encoder_fwd_pair_supported(self.cfg_train)     # eval + train forward as one two-segment pass
        n_saved, _ = ops.enc_sizes(self.cfg_train)
        self.hcfg_train = HeadCfg(self.T, E, net.D1, net.D2, net.kind, net.p_head, 1)
        self.hcfg_eval = HeadCfg(self.T, E, net.D1, net.D2, net.kind, net.p_head, 0)
        h_saved, _ = ops.head_sizes(self.hcfg_train)
        Do = net.D2 if net.kind == 0 else 1
        self.enc_out = self._enc_out[:self.T * E].view(S, B, E)
        self.saved = self._saved[:n_saved] if self.need_bwd else None
        self.hsaved = self._hsaved[:h_saved]
        self.out = self._out[:self.T * Do].view(S, B, Do)
        self.dx = self._dx[:self.T * E].view(S, B, E) if self.need_bwd else None


class _Res:
    """A resource touched by sub-steps on different HIP streams (a network's parameter slab, a pass buffer):
    the event of its last writer and the events of the readers since then."""

    def __init__(self):
        self.last_write = None
        self.reads = []


# Sub-step -> stream map for n_streams = 2: the visual generator's chain (the long pole: its two D steps and two
# G steps are 45 % of the work) runs beside everything else; dependencies are enforced by events, so any map is
# correct — this one balances the two streams (tools: see DESIGN.md §4).
STREAM_MAP = {1: [0] * 12,
              2: [0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1],     # measured best of six 2-stream maps (60.9 ms vs 81.6 ms on 1)
              3: [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 2, 2]}     # visual generator's chain on its own stream: 49.9 ms

# Bi-modal schedule of the MELD-dimension extension workload (BASELINE.json configs[2]; MELD has text and audio only,
# dataloader.py:93-95): the text/acoustic sub-steps 5-8 of the reference's order (train_IEMOCAP.py:363-370).
ADDS_PER_SUBSTEP = 4     # dropout-bearing launches of one sub-step (two encoder passes and two heads)
SCHEDULE_BIMODAL = [s for s in SCHEDULE if "visual" not in s[1:]]
STREAM_MAP_BIMODAL = {1: [0, 0, 0, 0], 2: [0, 0, 1, 1]}


# Widths up to this stay unpaired by default (GANFFN_GEN_PAIR=all pairs them too): the d_model-100 generators' sub-steps are not
# on the iteration's longest chain, and their paired launches measured slower in the three-stream step (DESIGN.md section 6,
# profiles/gen_pair_ab.txt); the 512-wide generator's chain is the longest, and its pairing shortens it.
GEN_PAIR_MAX_UNPAIRED_E = 128


def find_gen_pairs(schedule, stream_map):
    """sub-steps i whose generator forward can carry the next sub-step's: i = (D, ., p) runs generator p in eval mode on
    batch[p], i + 1 = (G, p, .) runs it in train mode on the same input, and only a discriminator is updated in between, so
    both passes see the same parameters.  Both sub-steps must be on the same stream.  -> sorted list of such i"""
    return [i for i in range(len(schedule) - 1)
            if schedule[i][0] == "D" and schedule[i + 1][0] == "G" and schedule[i + 1][1] == schedule[i][2]
            and stream_map[i] == stream_map[i + 1]]


_STREAMS = {}


def _side_streams(dev, prios, tuner=None, work=1):
    """the side streams of a device, chosen once per process and shared by every engine built afterwards.

    Which hardware queue a new HIP stream lands on depends on how many streams the process created and used before
    (torch's pools, RCCL, other engines), and with it how well kernels of different streams overlap: the same three
    sub-step chains ran at 34.7, 37.1, 40.5, 43.5 or 54 ms per iteration depending on nothing but that
    (tools/lab/stream_order.py; 1-workgroup spin kernels overlap on every pair — only real launch mixes tell the pairs
    apart).  `tuner(prios)` picks the streams by timing the asking engine's probe work (its _tune_slot) on fresh candidates
    (_NetRunner._tune_streams); without it, or with GANFFN_STREAM_TUNE=0, fresh streams are taken as they come; `work` =
    tokens per pass of the engine that asks (the choice is re-timed when a much bigger engine comes along).
    Sharing the streams between the engines of one process is safe for engines over DIFFERENT networks and buffers (each
    engine orders its own sub-steps with its own events).  Two engines over the SAME networks see only their own dependency
    records: DrnnEngine joins its streams at the end of every step, but an eager multi-stream GanEngine does not (consecutive
    iterations overlap) — call `eng.synchronize()` (or `loss_dict()`) before another engine touches the same networks
    (tests/test_hip_engine.py::test_two_engines_over_the_same_networks_need_a_synchronize)."""
    key = (str(dev), tuple(prios))
    if os.environ.get("GANFFN_STREAM_CACHE", "1") == "1" and key in _STREAMS and work <= 4 * _STREAMS[key][1]:
        return _STREAMS[key][0]                 # (a choice timed on a much smaller batch is not trusted for a big one)
    # (no timing probes while the caller is capturing a graph: they synchronise)
    if tuner is not None and len(prios) > 1 and os.environ.get("GANFFN_STREAM_TUNE", "1") == "1" and \
            not torch.cuda.is_current_stream_capturing():
        streams = tuner(prios)
    else:
        streams = [torch.cuda.Stream(device=dev, priority=p_) for p_ in prios]
    _STREAMS[key] = (streams, max(1, work))
    return streams


class _Runner:
    """what all four step runners share: the device, its RNG, the process group, the grow-only capacity of the step buffers
    (reserve / _fit), the check that no network re-packed its slab, and predictions.
      _Runner -> MeldEngine                                    (one slab, no generator)
      _Runner -> _NetRunner -> GanEngine, Phase2Engine, DrnnEngine
    _NetRunner holds the forward / backward / Adam of one network on preallocated pass buffers; the sub-step schedule, the
    stream map and the cross-stream dependency records are GanEngine's alone."""

    def _init_common(self, device, process_group, n_buckets, nets=()):
        self.dev = device
        self.rng = ops.DeviceRng.get(device)
        self.pg = process_group
        self.world = 1
        if process_group is not None:
            import torch.distributed as dist
            self.world = dist.get_world_size(process_group)
        self.n_buckets = n_buckets
        self._nets = list(nets)                  # [(name, NetState)]: what _check_slabs watches
        self._shape = None
        self._cap_S = self._cap_B = 0            # asked for (reserve) or seen so far
        self._alloc_S = self._alloc_B = 0        # what the buffers are sized for
        self._base_add = 0
        self._adds = 0

    def _check_slabs(self):
        """the engine trains the slab it captured at construction; a module that re-packed into a NEW slab since then
        (`.to(other device)`, `.double()`, load into fresh parameters) would silently stop following — refuse instead"""
        for k, st in self._nets:
            if st.m.slab.data_ptr() != st.slab.data_ptr():
                raise RuntimeError("network %r re-packed its parameters after the engine was built (module.slab moved): "
                                   "build the engine after the last .to()/.cuda()/dtype change" % k)

    def _check_SB(self, S, B):
        """engines with limits on a step's shape raise ValueError here"""

    def reserve(self, S, B):
        """size every step buffer once for dialogues of up to S utterances and batches of up to B dialogues, so that
        the varying (S, B) of real loaders (no drop_last: every epoch ends on a short batch, train_IEMOCAP.py:62-100;
        train / valid / test loaders differ) never touches the allocator again"""
        self._check_SB(S, B)
        self._cap_S, self._cap_B = max(self._cap_S, S), max(self._cap_B, B)

    def _fit(self, *shape, grow=False):
        """the capacity rule of every engine's prepare, for the step shape (S, B, ...) -> "same": the shape of the last step,
        nothing to do; "fits": within what the buffers were sized for — the caller takes new views, no allocation, no sync;
        "grow": the caller allocates for (_alloc_S, _alloc_B), which is the largest S and the largest B reserved or seen so
        far — capacity only ever grows (a short last batch must not shrink it).  grow=True: the caller outgrew a dimension
        of its own (DrnnEngine's party count).
        The new shape and allocation are recorded HERE, before the caller allocates (as GanEngine always did): an engine whose
        allocation raised (out of memory) is not fit to step again — build a new one."""
        if self._shape == shape:
            return "same"
        S, B = shape[:2]
        self._check_SB(S, B)
        self._shape = shape
        if not grow and S <= self._alloc_S and B <= self._alloc_B:
            return "fits"
        self._alloc_S = self._cap_S = max(self._cap_S, S)
        self._alloc_B = self._cap_B = max(self._cap_B, B)
        return "grow"

    predictions = staticmethod(predictions)


class _NetRunner(_Runner):
    """the network-level operations GanEngine, Phase2Engine and DrnnEngine share: forward, backward, all-reduce and Adam of ONE
    network (a NetState) on preallocated pass buffers (_Pass) with the workspace `self.ws`, dropout offsets relative to
    `_base_add`, and the timing of candidate side streams on the engine's own `_tune_slot`.  One stream and one communicator
    are the defaults here; GanEngine, whose sub-steps run on several streams, overrides `_cur_pg`, `_communicators` and
    `_pre_write`."""
    _cur_pg = None               # the communicator of the sub-step being issued (None: self.pg)
    # int32 [B] key lengths of the step being issued (Phase2Engine / DrnnEngine with mask_padding: the generators' self-attention
    # ignores padded utterances), or None: the plain encoder calls.  Held here until the next step replaces it, so the tensor
    # outlives the backward that reads it.  GanEngine, whose passes have two batch widths, overrides _pass_key_len instead.
    _key_len = None
    # causal self-attention in every encoder call of _net_fwd / _net_bwd (Phase2Engine(causal=True)); False: the calls without it.
    # GanEngine, whose discriminators stay bidirectional, chooses per network instead: it overrides _net_causal.
    _causal = False

    def _net_causal(self, net):
        """do the encoder calls on this network carry the causal flag?"""
        return self._causal

    def _pass_key_len(self, ps):
        """the key lengths of a forward / backward on the pass buffers ps (None: the plain encoder calls)"""
        return self._key_len

    def _communicators(self):
        """every communicator the engine issues collectives on"""
        return [self.pg]

    def _pre_write(self, net_key):
        """called right before a network's Adam; one stream: nothing to wait for"""

    def _next_add(self):
        v = self._adds
        self._adds += 1
        return self._base_add + v

    def _net_fwd(self, net, ps, x, train, save, adds=None):
        """encoder + head forward into ps.out; returns (enc_add, head_add) rng offsets used.  adds: the two dropout
        offsets (relative to the iteration's block) when the caller assigns them by sub-step; else the next two."""
        cfg = ps.cfg_train if train else ps.cfg_eval
        hcfg = ps.hcfg_train if train else ps.hcfg_eval
        if adds is None:
            a0, a1 = self._next_add(), self._next_add()
        else:
            a0, a1 = self._base_add + adds[0], self._base_add + adds[1]
        ops.encoder_fwd_raw(cfg, x, net.pe, net.slab, ps.enc_out, ps.saved if save else None, self.ws, self.rng.state, a0,
                            key_len=self._pass_key_len(ps), causal=self._net_causal(net))
        w = net.w
        w3 = w("fc3.weight") if net.kind == 1 else None
        b3 = w("fc3.bias") if net.kind == 1 else None
        ops.head_fwd_raw(hcfg, ps.enc_out, w("fc1.weight"), w("fc1.bias"), w("fc2.weight"), w("fc2.bias"), w3, b3,
                         ps.out, ps.hsaved, self.ws, self.rng.state, a1)
        return a0, a1

    def _net_bwd(self, net, ps, d_out, train, adds, want_wgrad, reduce_cb=None, need_dx=None, parts=False):
        """head + encoder backward; ps.dx <- dL/d(network input) when `need_dx` (default: exactly when the network is the
        frozen one that only passes gradient through).  Weight grads accumulate into net.grad."""
        cfg = ps.cfg_train if train else ps.cfg_eval
        hcfg = ps.hcfg_train if train else ps.hcfg_eval
        a0, a1 = adds
        w = net.w
        g = (lambda n: net.w(n, grad=True)) if want_wgrad else (lambda n: None)
        w3 = w("fc3.weight") if net.kind == 1 else None
        ops.head_bwd_raw(hcfg, d_out, ps.enc_out, w("fc1.weight"), w("fc2.weight"), w3,
                         g("fc1.weight"), g("fc1.bias"), g("fc2.weight"), g("fc2.bias"),
                         g("fc3.weight") if net.kind == 1 else None, g("fc3.bias") if net.kind == 1 else None,
                         ps.dx, ps.hsaved, self.ws, self.rng.state, a1)
        gslab = net.grad if want_wgrad else None
        # the network being trained reads a raw modality or detached fakes: nobody consumes dL/d(its input)
        # (train_IEMOCAP.py:200-252) — except the visual discriminator's `object` layer; the frozen discriminator of
        # train_gen passes its input gradient on to the generator
        if need_dx is None:
            need_dx = not want_wgrad
        if parts and want_wgrad and reduce_cb is None:
            # single GPU, d_model 100: the weight gradients stay as token-chunk slabs for Adam to add (no reduce launch, and the
            # caller did not zero the encoder region of net.grad) -> (parts view of self.ws, stride, chunks)
            return ops.encoder_bwd_parts_raw(cfg, ps.dx, net.slab, gslab, ps.saved, self.ws, self.rng.state, a0, need_dx,
                                             key_len=self._pass_key_len(ps), causal=self._net_causal(net))
        if reduce_cb is None or not want_wgrad:
            ops.encoder_bwd_raw(cfg, 0, net.L, ps.dx, net.slab, gslab, ps.saved, self.ws, self.rng.state, a0, need_dx,
                                key_len=self._pass_key_len(ps), causal=self._net_causal(net))
        else:
            # bucketed: backward a group of layers, then hand that slice of the grad slab to the all-reduce
            bks = net.buckets(self.n_buckets)
            reduce_cb(*bks[0], last=False)                       # head (+object handled by caller before this)
            for i, (lo_f, hi_f) in enumerate(bks[1:]):
                lo, hi = lo_f // net.layer_floats, hi_f // net.layer_floats
                ops.encoder_bwd_raw(cfg, lo, hi, ps.dx, net.slab, gslab, ps.saved, self.ws, self.rng.state, a0, need_dx,
                                    key_len=self._pass_key_len(ps), causal=self._net_causal(net))
                reduce_cb(lo_f, hi_f, last=(i == len(bks) - 2))

    def _adam(self, net, parts=None):
        if parts is not None and parts[2] > 1:
            ops.adam_step_parts_raw(net.slab, net.grad, net.exp_avg, net.exp_avg_sq, net.step, net.total, net.lr, net.betas[0],
                                    net.betas[1], parts[0], parts[1], parts[2], net.enc_floats, net.layer_floats, net.covered,
                                    1e-8, net.wd, 1.0 / self.world)
            return
        ops.adam_step_raw(net.slab, net.grad, net.exp_avg, net.exp_avg_sq, net.step, net.total, net.lr,
                          net.betas[0], net.betas[1], 1e-8, net.wd, 1.0 / self.world)

    def _adam_slice(self, net, lo, hi):
        ops.adam_update_raw(net.slab[lo:hi], net.grad[lo:hi], net.exp_avg[lo:hi], net.exp_avg_sq[lo:hi], net.step, hi - lo,
                            net.lr, net.betas[0], net.betas[1], 1e-8, net.wd, 1.0 / self.world)

    def _parts_ok(self, net, ps):
        """single GPU, d_model 100: leave the weight gradients of this backward pass as token-chunk slabs and let Adam add them
        (ganffn_encoder_bwd_parts / ganffn_adam_step_parts): no reduce launch, no zero-fill of the encoder region of net.grad.
        With a process group the all-reduce needs the summed slab: today's path.  GANFFN_ADAM_PARTS=0 switches it off."""
        return self.pg is None and os.environ.get("GANFFN_ADAM_PARTS", "1") == "1" and net.total % 4 == 0 and \
            ops.encoder_bwd_parts_supported(ps.cfg_train)

    def _zero_grad(self, net, parts):
        """opt.zero_grad() (train_IEMOCAP.py:216,245); with unreduced weight gradients only what still accumulates: heads, `object`"""
        if parts:
            net.grad[net.enc_floats:].zero_()
        else:
            net.grad.zero_()

    def _make_reducer(self, net):
        """returns (callback, finish_and_step): async all-reduce (sum) of grad-slab slices on RCCL's own stream,
        overlapping the rest of backward.  finish_and_step(net_key) waits bucket by bucket and applies Adam (which
        divides by world: grad_scale) to each slice as soon as its reduce is done; without a process group it is the
        plain whole-slab Adam step."""
        if self.pg is None:
            def plain(net_key, parts=None):
                self._pre_write(net_key)
                self._adam(net, parts)
            return None, plain
        if dp_mode() == "inline":
            import torch.distributed as dist
            group = self._cur_pg or self.pg

            def inline(net_key, parts=None):
                # on the CURRENT stream (the sub-step's own): sum over ranks, then Adam divides by world (grad_scale)
                dist.all_reduce(net.grad, op=dist.ReduceOp.SUM, group=group, async_op=False)
                self._pre_write(net_key)
                self._adam(net)
            return None, inline
        red = GradReducer(self._cur_pg or self.pg)

        def cb(lo, hi, last):
            red.reduce_async(net.grad[lo:hi], lo, hi)

        def finish_and_step(net_key, parts=None):
            self._pre_write(net_key)            # other streams' readers of these parameters first (WAR)
            red.finish(lambda lo, hi: self._adam_slice(net, lo, hi) if hi > lo else None)
            ops.adam_bump_raw(net.step)
        return cb, finish_and_step

    def _tune_streams(self, prios, n_cand=6, reps=2):
        """choose one stream per entry of `prios` among n_cand fresh candidates per priority by TIMING them on this engine's
        own kernels: slot i runs _tune_slot(i) beside the slots already chosen; the first two slots are chosen jointly over
        all candidate pairs, every further slot greedily.  ~0.15 s, once per process and device."""
        dev = self.dev
        n_cand = int(os.environ.get("GANFFN_STREAM_CAND", n_cand))
        cands = {p_: [torch.cuda.Stream(device=dev, priority=p_) for _ in range(n_cand)] for p_ in sorted(set(prios))}
        cur = torch.cuda.current_stream(dev)

        def probe(streams):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            for i, st in enumerate(streams):
                st.wait_event(e0)
                with torch.cuda.stream(st):
                    self._tune_slot(i)
            for st in streams:
                cur.wait_stream(st)
            e1.record(cur)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def best(fixed, pool):
            timed = []
            for c_ in pool:
                group = fixed + (list(c_) if isinstance(c_, tuple) else [c_])
                timed.append((min(probe(group) for _ in range(reps)), c_))
            return min(timed, key=lambda t_: t_[0])[1]

        if self.pg is not None:
            # RCCL creates its internal stream(s) at the first collective of a communicator; a stream that appears AFTER the
            # choice below can land on a hardware queue one of the chosen streams uses.  Issue one tiny all-reduce per
            # communicator first, so that the candidates are timed with RCCL's queue already taken.
            for g_ in self._communicators():
                if g_ is not None:
                    self.dist_warm = torch.zeros(8, device=dev)
                    import torch.distributed as dist
                    dist.all_reduce(self.dist_warm, group=g_, async_op=(dp_mode() != "inline"))
                    if dp_mode() != "inline":
                        torch.cuda.synchronize(dev)
        torch.cuda.synchronize(dev)
        saved_add = self._base_add
        self._base_add = 0
        try:
            probe([cands[prios[0]][0]])                                      # warm-up (lazy module / allocator state)
            if prios[0] == prios[1]:
                pool = [(a_, b_) for i, a_ in enumerate(cands[prios[0]]) for b_ in cands[prios[0]][i + 1:]]
            else:
                pool = [(a_, b_) for a_ in cands[prios[0]] for b_ in cands[prios[1]]]
            chosen = list(best([], pool))
            for p_ in prios[2:]:
                chosen.append(best(chosen, [c_ for c_ in cands[p_] if c_ not in chosen]))
        finally:
            self._base_add = saved_add
            torch.cuda.synchronize(dev)
        return chosen


class GanEngine(_NetRunner):
    """train_GAN's inner loop (train_IEMOCAP.py:320-382) for a fixed batch shape.

    n_streams > 1: independent sub-steps run concurrently on several HIP streams.  The 12 sub-steps form a
    DAG over the six networks (e.g. (D_t|G_a) only needs G_a from sub-step 2 and can run beside
    (D_v|G_t)/(G_t|D_v)); every sub-step waits for the writers of what it reads and, before its Adam, for
    the readers of what it writes — so each one sees exactly the parameter versions of the sequential
    schedule.  Most kernels of this workload fill a fraction of the 256 CUs, so overlapping them is free.

    mask_padding (default False: the reference passes no mask and averages its losses over every padded position) is an
    extension: iteration(batch) reads batch["umask"] [B, S]; every generator and discriminator pass of every sub-step attends
    over the real utterances of its dialogue only (key lengths = umask.sum(1), computed and kept on the device; a discriminator's
    [real | fake] pass of 2B dialogues gets them twice), and both losses are means over the real utterances (ganffn_bce_len).
    Padded rows then get a loss gradient of exactly 0, so finite values at padded positions of the batch change no bit of any
    loss, gradient or updated parameter.  Under a process group each rank divides by its OWN count of real utterances: the
    all-reduced gradient is the mean of the ranks' masked means (as the reference's is the mean of their padded means), not the
    mean over all ranks' utterances.  GANFFN_CHECK_QMASK=1 checks that umask rows are prefixes (one host sync per batch).  Off,
    the engine issues exactly the calls it issued before the option existed.

    causal (default False: the reference's generators are bidirectional) is an extension too: every GENERATOR pass of every
    sub-step — the eval-mode forward of a discriminator sub-step, the train-mode forward and backward of a generator sub-step,
    both segments of a paired forward — runs under the causal mask (query i attends to keys j <= i; with mask_padding
    j < min(len, i + 1)), so the generators are trained in the regime a streaming classifier runs them in.  The DISCRIMINATORS
    stay bidirectional: they are training-time critics of whole fused sequences and are never deployed, so every discriminator
    launch is the one issued without the option.  Dropout offsets, the Philox indexing, the stream map, the pairing rule and the
    parts rule are unchanged; it composes with mask_padding, graph capture, several streams and a process group.  Off, the
    engine issues exactly the calls it issued before the option existed."""

    def __init__(self, gens, discs, lr=1e-4, b1=0.5, b2=0.6, process_group=None, n_buckets=3, use_graph=False,
                 n_streams=1, schedule=None, mask_padding=False, causal=False):
        self.mask_padding = bool(mask_padding)
        self.causal = bool(causal)
        self._kl1 = self._kl2 = None         # int32 key lengths of the iteration being issued: [B], and [2B] = the same twice
        # optimizers: train_IEMOCAP.py:292-297 (G lr, text-G 1.1*lr, every D lr/2); call site :603-606
        self.G = {k: NetState(m, lr * (1.1 if k == "text" else 1.0), (b1, b2)) for k, m in gens.items()}
        self.D = {k: NetState(m, lr / 2, (b1, b2)) for k, m in discs.items()}
        self._init_common(next(iter(self.G.values())).slab.device, process_group, n_buckets,
                          list(self.G.items()) + list(self.D.items()))
        self.modalities = list(self.G.keys())
        if schedule is None:
            schedule = SCHEDULE if set(self.modalities) == {"acoustic", "visual", "text"} else \
                [s_ for s_ in SCHEDULE if s_[1] in self.G and s_[2] in self.G]
        self.schedule = list(schedule)
        self.D_h = next(iter(self.G.values())).D2          # width of the fused feature = every discriminator's d_model
        stream_maps = STREAM_MAP if len(self.schedule) == 12 else \
            {1: [0] * len(self.schedule), 2: [(i // 2) % 2 for i in range(len(self.schedule))]}
        self.use_graph = use_graph
        if n_streams not in stream_maps:
            n_streams = max(k for k in stream_maps if k <= max(1, n_streams))
        self.n_streams = n_streams
        if use_graph and self.n_streams > 1:
            # multi-stream capture is not used: replay == eager here (the step is GPU-bound, not launch-bound), and
            # eager streams additionally overlap consecutive iterations
            self.use_graph = use_graph = False
        self.stream_map = stream_maps[self.n_streams]
        if os.environ.get("GANFFN_STREAM_MAP"):
            self.stream_map = [int(x) for x in os.environ["GANFFN_STREAM_MAP"].split(",")]
            assert len(self.stream_map) == len(self.schedule) and max(self.stream_map) < self.n_streams
        # eval + train generator forward of a (D, G) sub-step pair as one two-segment pass (ganffn_encoder_fwd_pair): on unless
        # GANFFN_GEN_PAIR=0.  GANFFN_GEN_PAIR=all pairs every stack that has a pair pass, 1 those that gained from it
        # (_pair_slot).  Unset: 1 in the multi-stream runner (the product's and the benchmark's mode, where the gain was
        # measured), 0 on one stream — there every sub-step issues its own generator forward with its own offsets, the launch
        # sequence the fp64 train-step oracle test walks sub-step by sub-step (tests/test_hip_engine_train_oracle.py); ask for
        # 1 or all to pair there too
        self.gen_pair_mode = os.environ.get("GANFFN_GEN_PAIR") or ("1" if self.n_streams > 1 else "0")
        self.gen_pair = self.gen_pair_mode != "0"
        self._gen_pairs = frozenset(find_gen_pairs(self.schedule, self.stream_map))
        self.streams = None
        self._cur_stream = None              # the stream of the sub-step being issued (multi-stream loop of _iteration_body)
        self._tune_x = (None, None)          # (shape, inputs) of _tune_slot's probe work
        self._res = {}
        # One communicator per sub-step stream (default in the in-line mode, see dp_mode(); GANFFN_COMM_PER_STREAM overrides).
        self.pgs = [process_group]
        per_stream = os.environ.get("GANFFN_COMM_PER_STREAM", "1" if dp_mode() == "inline" else "0") == "1"
        if process_group is not None and self.n_streams > 1 and not per_stream and dp_mode() == "inline":
            import torch.distributed as dist
            if dist.get_backend(process_group) == "nccl":
                # in-line collectives of different sub-step streams would share ONE RCCL communicator and may be in flight
                # together: RCCL (like NCCL) does not support that.  (gloo reduces on the host, synchronously: no such limit.)
                raise RuntimeError("GANFFN_DP_MODE=inline with %d sub-step streams needs one communicator per stream: "
                                   "leave GANFFN_COMM_PER_STREAM at 1, or use n_streams=1, or GANFFN_DP_MODE=buckets" % self.n_streams)
        # Ordering assumption of the in-line mode: every rank runs the SAME host program, so the
        # collectives of the three communicators are issued in the same host order on every rank; whatever order a rank's
        # hardware queues impose is a sub-order of that one, so no two ranks can wait on each other's collectives in a cycle.
        # Never measured on more than one rank (no multi-GPU node was available): `python bench.py --gpus N` therefore runs
        # under a watchdog that falls back to one stream / one communicator and then to the bucket mode.
        if process_group is not None and self.n_streams > 1 and per_stream:
            # in-line collectives run on the sub-step streams themselves; two of them may be in flight at once, and one
            # communicator must never carry two collectives concurrently: one communicator per sub-step stream (every rank
            # creates them here, in the same order; each stream's collectives are ordered by the stream)
            import torch.distributed as dist
            ranks = list(range(dist.get_world_size(process_group)))
            self.pgs += [dist.new_group(ranks=ranks) for _ in range(self.n_streams - 1)]
        self._cur_pg = process_group
        self._graph = None
        self.losses = torch.zeros(len(self.schedule), device=self.dev)

    def _communicators(self):
        return self.pgs

    def _net_causal(self, net):
        return self.causal and net.kind == 0         # the generators; a discriminator (kind 1) judges the whole sequence

    def _pass_key_len(self, ps):
        if self._kl1 is None:
            return None
        return self._kl2 if ps.B == self._kl2.numel() else self._kl1

    # ------------------------------------------------------------------------------------------
    def _prepare(self, S, B):
        first = self._shape is None
        fit = self._fit(S, B)
        if fit == "same":
            return
        self._graph = None
        self.static_batch = None
        if fit == "fits":
            # new views, no allocation, no sync.  (A pass of fewer dialogues uses a prefix of the flat storage; layouts are
            # derived from (S, B) alone.)
            self._resize_passes(S, B)
            self._view_scratch(S, B)
            return
        if not first and self.n_streams > 1:
            # the buffers about to be dropped may still be in use by sub-steps queued on the side streams (eager
            # iterations overlap); the caching allocator only tracks the allocating stream
            torch.cuda.synchronize(self.dev)
        cS, cB, dev = self._alloc_S, self._alloc_B, self.dev
        self.pass_G_nosave = {k: _Pass(n, cS, cB, dev, False) for k, n in self.G.items()}
        self.pass_G = {k: _Pass(n, cS, cB, dev, True) for k, n in self.G.items()}
        self.pass_D2 = {k: _Pass(n, cS, 2 * cB, dev, True) for k, n in self.D.items()}   # [real | fake]
        self.pass_D1 = {k: _Pass(n, cS, cB, dev, True) for k, n in self.D.items()}       # frozen D in train_gen
        n_ws = max(p.n_ws for d in (self.pass_G, self.pass_D2, self.pass_D1, self.pass_G_nosave) for p in d.values())
        f32 = dict(device=dev, dtype=torch.float32)
        Dh = self.D_h
        # scratch is per stream (sub-steps on different streams run concurrently); flat, viewed per (S, B)
        self._scratch_flat = [dict(ws=torch.empty(n_ws, **f32), x_cat=torch.empty(cS * 2 * cB * Dh, **f32),
                                   obj_out=torch.empty(cS * cB * Dh, **f32), dprob2=torch.empty(cS * 2 * cB, **f32),
                                   dprob1=torch.empty(cS * cB, **f32), d_real=torch.empty(cS * cB * Dh, **f32))
                              for _ in range(self.n_streams)]
        if (S, B) != (cS, cB):
            self._resize_passes(S, B)
        self._view_scratch(S, B)
        if self.n_streams > 1 and self.streams is None:
            # stream priorities: the visual generator's chain (stream 2 of the 3-stream map: its four sub-steps are a cycle
            # through G_v's parameters and pace the iteration) gets the high priority — measured 35.34 -> 34.90 ms per step
            # (GANFFN_STREAM_PRIO="0,0,0" restores equal priorities; "-1,-1,0" measured 35.6)
            default_prio = "0,0,-1" if (self.n_streams == 3 and len(self.schedule) == 12) else ""
            prio = [int(x) for x in os.environ.get("GANFFN_STREAM_PRIO", default_prio).split(",") if x.strip()]
            prio = (prio + [0] * self.n_streams)[:self.n_streams]
            self.streams = list(_side_streams(dev, prio, self._tune_streams, S * B))
            self._tune_x = (None, None)
            self._use_scratch(0)
        self._res = {}

    def _tune_slot(self, i):
        """the probe work of stream slot i for _tune_streams: eval-mode forwards of one generator into its no-save pass
        buffers with the slot's scratch (nothing else is written: no parameter, gradient or RNG state changes)"""
        k = self.modalities[i % len(self.modalities)]
        if self._tune_x[0] != self._shape:
            S, B = self._shape
            self._tune_x = (self._shape, {m: torch.zeros(S, B, self.G[m].E, device=self.dev) for m in self.modalities})
        self._use_scratch(i)
        for _ in range(1 if self.G[k].E > 256 else 3):                      # (the 512-wide generator is ~3x a 100-wide one)
            self._net_fwd(self.G[k], self.pass_G_nosave[k], self._tune_x[1][k], train=False, save=False, adds=(0, 1))

    def _resize_passes(self, S, B):
        for d in (self.pass_G_nosave, self.pass_G, self.pass_D1):
            for p_ in d.values():
                p_.resize(S, B)
        for p_ in self.pass_D2.values():
            p_.resize(S, 2 * B)

    def _view_scratch(self, S, B):
        Dh = self.D_h
        self.scratch = [dict(ws=f["ws"], x_cat=f["x_cat"][:S * 2 * B * Dh].view(S, 2 * B, Dh),
                             obj_out=f["obj_out"][:S * B * Dh].view(S, B, Dh),
                             dprob2=f["dprob2"][:S * 2 * B].view(S, 2 * B, 1), dprob1=f["dprob1"][:S * B].view(S, B, 1),
                             d_real=f["d_real"][:S * B * Dh].view(S, B, Dh)) for f in self._scratch_flat]
        self._use_scratch(0)

    def _use_scratch(self, i):
        sc = self.scratch[i]
        self.ws, self.x_cat, self.obj_out = sc["ws"], sc["x_cat"], sc["obj_out"]
        self.dprob2, self.dprob1, self.d_real = sc["dprob2"], sc["dprob1"], sc["d_real"]

    # ---- cross-stream dependencies -------------------------------------------------------------
    def _r(self, key):
        r = self._res.get(key)
        if r is None:
            r = self._res[key] = _Res()
        return r

    def _wait_writers(self, stream, keys):
        for k in keys:
            ev = self._r(k).last_write
            if ev is not None:
                stream.wait_event(ev)

    def _wait_readers(self, stream, keys):
        for k in keys:
            for ev in self._r(k).reads:
                stream.wait_event(ev)

    def _done(self, stream, reads, writes):
        ev = torch.cuda.Event()
        ev.record(stream)
        for k in reads:
            self._r(k).reads.append(ev)
        for k in writes:
            r = self._r(k)
            r.last_write, r.reads = ev, []

    # ------------------------------------------------------------------------------------------
    def _gen_pair_fwd(self, net, ps_eval, ps_train, x, adds_eval, adds_train):
        """the eval-mode forward (into ps_eval, nothing saved) and the train-mode forward (into ps_train, saved) of one
        generator over x: one two-segment encoder pass, then the two heads; -> the train pass's (enc_add, head_add)"""
        a0, a1 = self._base_add + adds_train[0], self._base_add + adds_train[1]
        ops.encoder_fwd_pair_raw(ps_train.cfg_train, x, net.pe, net.slab, ps_eval.enc_out, ps_train.enc_out, ps_train.saved,
                                 self.ws, self.rng.state, a0, key_len=self._pass_key_len(ps_train), causal=self._net_causal(net))
        w = net.w
        w3 = w("fc3.weight") if net.kind == 1 else None
        b3 = w("fc3.bias") if net.kind == 1 else None
        for hcfg, ps, add in ((ps_eval.hcfg_eval, ps_eval, self._base_add + adds_eval[1]), (ps_train.hcfg_train, ps_train, a1)):
            ops.head_fwd_raw(hcfg, ps.enc_out, w("fc1.weight"), w("fc1.bias"), w("fc2.weight"), w("fc2.bias"), w3, b3,
                             ps.out, ps.hsaved, self.ws, self.rng.state, add)
        return a0, a1

    def _pair_slot(self, i):
        """the sub-step whose train-mode generator forward sub-step i (a discriminator step) issues with its own eval-mode
        one, or None"""
        if not self.gen_pair or i not in self._gen_pairs:
            return None
        ps = self.pass_G[self.schedule[i][2]]
        if not ps.pair_ok or (self.gen_pair_mode != "all" and ps.net.E <= GEN_PAIR_MAX_UNPAIRED_E):
            return None
        return i + 1

    def train_disc(self, who, partner, batch, loss_slot, pair_slot=None):
        """train_IEMOCAP.py:200-227.  pair_slot: the next sub-step trains `partner` on the same input — its train-mode forward
        is issued here, in the launches of the eval-mode one, with that sub-step's dropout offsets; -> its g_adds (else None)"""
        S, B = batch[who].shape[:2]
        Dn, Gn = self.D[who], self.G[partner]
        pg_, pd = self.pass_G_nosave[partner], self.pass_D2[who]
        # dropout offsets are assigned by sub-step (4 per sub-step: generator encoder / head, discriminator encoder / head), so
        # they do not depend on the order in which streams issue their launches
        a = ADDS_PER_SUBSTEP * loss_slot
        # fusion = G(real_gen) in eval mode, nothing saved (detach(), :218-219)
        g_adds = None
        if pair_slot is not None:
            ap = ADDS_PER_SUBSTEP * pair_slot
            g_adds = self._gen_pair_fwd(Gn, pg_, self.pass_G[partner], batch[partner], (a, a + 1), (ap, ap + 1))
        else:
            self._net_fwd(Gn, pg_, batch[partner], train=False, save=False, adds=(a, a + 1))
        # real input of D_m is raw modality m; VisualDiscriminator maps 512 -> 100 first (model.py:1355-1356)
        x_real = batch[who]
        if Dn.has_obj:
            ops.linear_fwd_raw(x_real, Dn.w("object.weight"), Dn.w("object.bias"), self.obj_out, S * B, Dn.obj_in, self.D_h)
            x_real = self.obj_out
        torch.cat((x_real, pg_.out), dim=1, out=self.x_cat)
        adds = self._net_fwd(Dn, pd, self.x_cat, train=True, save=True, adds=(a + 2, a + 3))
        n = S * 2 * B
        if self._kl1 is not None:
            # the mean over real utterances only; the real and the fake half have the same lengths (key_len[c % B])
            ops.bce_len_fwd_raw(pd.out, self._kl1, B, 1.0, 0.0, S, 2 * B, B, 1.0, self.losses[loss_slot:loss_slot + 1], False)
            ops.bce_len_bwd_raw(pd.out, self._kl1, B, 1.0, 0.0, S, 2 * B, B, 1.0, self.dprob2)
        else:
            ops._lib.call("ganffn_bce2_fwd", ops._ptr(pd.out), C.c_float(1.0), C.c_float(0.0), 2 * B, B, n, C.c_float(1.0),
                          ops._ptr(self.losses[loss_slot:loss_slot + 1]), 0, ops._stream())
            ops._lib.call("ganffn_bce2_bwd", ops._ptr(pd.out), C.c_float(1.0), C.c_float(0.0), 2 * B, B, n, C.c_float(1.0),
                          ops._ptr(self.dprob2), ops._stream())
        parts_mode = self._parts_ok(Dn, pd)
        self._zero_grad(Dn, parts_mode)                              # opt.zero_grad(), :216
        cb, finish = self._make_reducer(Dn)
        parts = self._net_bwd(Dn, pd, self.dprob2, True, adds, True, cb, need_dx=Dn.has_obj, parts=parts_mode)
        if Dn.has_obj:
            self.d_real.copy_(pd.dx[:, :B])                      # gradient of the real half of the batch
            # (scratch: the workspace BELOW the unreduced weight-gradient chunks the Adam launch is about to read)
            scratch = self.ws[:parts[3]] if (parts is not None and parts[2] > 1) else self.ws
            ops.linear_bwd_raw(self.d_real, batch[who], Dn.w("object.weight"), None, Dn.w("object.weight", True),
                               Dn.w("object.bias", True), S * B, Dn.obj_in, self.D_h, scratch)
            if cb is not None:
                cb(Dn.enc_floats, Dn.enc_floats + Dn.obj_floats, last=True)
        finish(("D", who), parts)
        return g_adds

    def train_gen_forward(self, who, batch, loss_slot):
        """the generator's own forward of train_gen (train mode, saved for backward): it reads nothing but the generator's
        parameters and the batch (a paired discriminator sub-step issues it instead, with its own eval-mode one: _gen_pair_fwd)"""
        a = ADDS_PER_SUBSTEP * loss_slot
        return self._net_fwd(self.G[who], self.pass_G[who], batch[who], train=True, save=True, adds=(a, a + 1))

    def train_gen(self, who, partner, batch, loss_slot, g_adds=None):
        """train_IEMOCAP.py:230-252.  g_adds: the generator forward has already been issued (train_gen_forward)."""
        S, B = batch[who].shape[:2]
        Gn, Dn = self.G[who], self.D[partner]
        pg_, pd = self.pass_G[who], self.pass_D1[partner]
        a = ADDS_PER_SUBSTEP * loss_slot
        if g_adds is None:
            g_adds = self.train_gen_forward(who, batch, loss_slot)
        d_adds = self._net_fwd(Dn, pd, pg_.out, train=False, save=True, adds=(a + 2, a + 3))       # disc.eval(), :243
        n = S * B
        if self._kl1 is not None:
            ops.bce_len_fwd_raw(pd.out, self._kl1, B, 1.0, 1.0, S, B, B, 1.0, self.losses[loss_slot:loss_slot + 1], False)
            ops.bce_len_bwd_raw(pd.out, self._kl1, B, 1.0, 1.0, S, B, B, 1.0, self.dprob1)
        else:
            ops.bce_fwd_raw(pd.out, 1.0, n, 1.0, self.losses[loss_slot:loss_slot + 1], False)
            ops.bce_bwd_raw(pd.out, 1.0, n, 1.0, self.dprob1)
        self._net_bwd(Dn, pd, self.dprob1, False, d_adds, False)             # through the frozen D: dgrad only
        parts_mode = self._parts_ok(Gn, pg_)
        self._zero_grad(Gn, parts_mode)
        cb, finish = self._make_reducer(Gn)
        parts = self._net_bwd(Gn, pg_, pd.dx, True, g_adds, True, cb, parts=parts_mode)
        finish(("G", who), parts)

    def _pre_write(self, net_key):
        """called right before a sub-step's Adam: wait for other streams' readers of that network (WAR)"""
        if self._cur_stream is not None:
            self._wait_readers(self._cur_stream, [net_key])

    # ------------------------------------------------------------------------------------------
    def _iteration_body(self, batch, device_rng_advance, lens=None):
        """lens: (int32 [B], int32 [2B]) key lengths of this batch on the device (mask_padding), or None"""
        self._adds = 0
        self._check_slabs()
        self._kl1, self._kl2 = lens if lens is not None else (None, None)
        if not device_rng_advance:
            # eager: this iteration's block of dropout offsets comes from the device's one allocator (shared with the
            # module path and every other engine); iterations may overlap, the offsets are host-side arguments
            self._base_add = self.rng.next_add(ADDS_PER_SUBSTEP * len(self.schedule))
        self._adds = ADDS_PER_SUBSTEP * len(self.schedule)       # (offsets are assigned by sub-step: train_disc / train_gen)
        paired = {}                      # sub-step -> (enc_add, head_add) of its generator forward, issued by the sub-step before
        if self.n_streams == 1:
            for i, (kind, who, partner) in enumerate(self.schedule):
                j = self._pair_slot(i) if kind == "D" else None
                if j is not None:
                    paired[j] = self.train_disc(who, partner, batch, i, pair_slot=j)
                elif kind == "D":
                    self.train_disc(who, partner, batch, i)
                elif i in paired:
                    self.train_gen(who, partner, batch, i, g_adds=paired[i])
                else:
                    self.train_gen(who, partner, batch, i)
        else:
            origin = torch.cuda.current_stream()
            fork = torch.cuda.Event()
            fork.record(origin)
            smap = self.stream_map
            for st in self.streams:
                st.wait_event(fork)
                # the caller may drop this batch as soon as we return while the side streams still read it: tell the
                # caching allocator, so the memory is not handed out again before those streams are done with it
                for k in self.modalities:
                    if batch[k].is_cuda:
                        batch[k].record_stream(st)
                for t_ in lens or ():
                    t_.record_stream(st)                     # computed on the caller's stream, read by every sub-step stream
            for i, (kind, who, partner) in enumerate(self.schedule):
                st = self.streams[smap[i]]
                trained = (kind, who)
                other = ("G" if kind == "D" else "D", partner)
                # pass buffers are resources too (same (net, role) buffer reused by a later sub-step)
                pj = self._pair_slot(i) if kind == "D" else None
                if kind == "D":
                    bufs = [("buf", "G_nosave", partner), ("buf", "D2", who)]
                    if pj is not None:
                        bufs.append(("buf", "G", partner))      # the paired pass writes the next sub-step's generator buffers
                else:
                    bufs = [("buf", "G", who), ("buf", "D1", partner)]
                self._use_scratch(smap[i])
                self._cur_stream = st
                self._cur_pg = self.pgs[smap[i]] if len(self.pgs) > 1 else self.pg
                with torch.cuda.stream(st):
                    self._wait_writers(st, [trained, other] + bufs)
                    self._wait_readers(st, bufs)
                    if kind == "D":
                        g_adds = self.train_disc(who, partner, batch, i, pair_slot=pj)
                        if pj is not None:
                            paired[pj] = g_adds
                    else:
                        self.train_gen(who, partner, batch, i, g_adds=paired.get(i))
                    self._done(st, reads=[other], writes=[trained] + bufs)
                self._cur_stream = None
            self._cur_pg = self.pg
            self._use_scratch(0)
            if device_rng_advance:
                # graph mode: join everything (the device-side offset bump below must follow every kernel)
                for st in self.streams:
                    origin.wait_stream(st)
                self._res = {}
        if device_rng_advance:
            ops.rng_advance_raw(self.rng.state, self._adds)
        else:
            assert self._adds <= ADDS_PER_SUBSTEP * len(self.schedule), self._adds

    def synchronize(self):
        """make the current stream wait for all side-stream work (call before reading results / timing)"""
        if self.n_streams > 1 and self.streams is not None:
            cur = torch.cuda.current_stream()
            for st in self.streams:
                cur.wait_stream(st)

    def iteration(self, batch):
        """One batch = 12 sub-steps.  Returns the device tensor of the 12 sub-step losses (no host sync).
        With n_streams > 1 call synchronize() (or loss_dict()) before reading it on the current stream."""
        S, B = batch[self.modalities[0]].shape[:2]
        self._kl1 = self._kl2 = None             # (the stream probe of _prepare runs plain forwards)
        self._prepare(S, B)
        lens = self._batch_lens(batch, S, B) if self.mask_padding else None
        if not self.use_graph:
            self._iteration_body(batch, device_rng_advance=False, lens=lens)
            return self.losses
        if self.static_batch is None:
            self.static_batch = {k: batch[k].clone() for k in self.modalities}
            if lens is not None:
                self.static_batch["key_len"], self.static_batch["key_len2"] = lens[0].clone(), lens[1].clone()
        else:
            for k in self.modalities:
                self.static_batch[k].copy_(batch[k])
            if lens is not None:
                self.static_batch["key_len"].copy_(lens[0])
                self.static_batch["key_len2"].copy_(lens[1])
        if lens is not None:
            lens = (self.static_batch["key_len"], self.static_batch["key_len2"])     # the addresses the graph was captured on
        if self._graph is None:
            # warm up on a side stream (allocations, lazy module init), then capture
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._iteration_body(self.static_batch, device_rng_advance=True, lens=lens)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._iteration_body(self.static_batch, device_rng_advance=True, lens=lens)
        self._graph.replay()
        return self.losses

    def _batch_lens(self, batch, S, B):
        """mask_padding: (key lengths [B], the same twice [2B]) from batch["umask"] [B, S], on the device, no host read"""
        umask = batch.get("umask") if hasattr(batch, "get") else None
        if umask is None:
            raise ValueError('GanEngine(mask_padding=True) needs batch["umask"] (batch, seq_len) to know every dialogue\'s length')
        if tuple(umask.shape) != (B, S):
            raise ValueError('batch["umask"] must be [%d, %d] (batch, seq_len), got %s' % (B, S, tuple(umask.shape)))
        if ops._CHECK_QMASK:
            ops.check_prefix_mask(umask, "GanEngine")
        kl = ops.key_lengths_from_umask(umask.to(self.dev)).contiguous()
        return kl, torch.cat((kl, kl))

    def loss_dict(self):
        """host copy of the last iteration's losses under the reference's column names (last value per key,
        as train_IEMOCAP.py:355-382 keeps)."""
        self.synchronize()
        v = self.losses.tolist()
        out = {}
        for (kind, who, _), x in zip(self.schedule, v):
            out["%s_%s_loss" % (who, kind)] = x
        return out


def build_networks(D_h=100, dropout=0.2, device="cuda", seed=None):
    """the six networks as train_IEMOCAP.py:580-585 builds them"""
    from . import model
    if seed is not None:
        torch.manual_seed(seed)
    discs = {"acoustic": model.AcousticDiscriminator(D_h, dropout=dropout),
             "visual": model.VisualDiscriminator(D_h, dropout=dropout),
             "text": model.TextDiscriminator(D_h, dropout=dropout)}
    gens = {"acoustic": model.AcousticGenerator(D_h, dropout=dropout),
            "visual": model.VisualGenerator(D_h, dropout=dropout),
            "text": model.TextGenerator(D_h, dropout=dropout)}
    for d in (gens, discs):
        for k in d:
            d[k] = d[k].to(device)
    return gens, discs


def train_GAN(gens, discs, batches, epochs=1, lr=1e-4, b1=0.5, b2=0.6, process_group=None, use_graph=False, log=None,
              n_streams=3, reserve_S=None, mask_padding=False, causal=False):
    """Counterpart of train_GAN (train_IEMOCAP.py:255-393) over an iterable of batches per epoch.
    Returns rows of the GAN_loss table (columns train_IEMOCAP.py:308-316): last batch of each epoch.
    reserve_S: size the step buffers once for dialogues up to this length (PositionalEncoding allows 110), so that
    batches of varying length never re-allocate.
    The losses are read on the host per batch only when `log` wants them; otherwise once per epoch (the last batch's).
    mask_padding: every batch carries "umask" [B, S]; attention and losses ignore padded utterances (GanEngine).
    causal: the generators' self-attention never looks ahead; the discriminators stay bidirectional (GanEngine)."""
    eng = GanEngine(gens, discs, lr, b1, b2, process_group, use_graph=use_graph, n_streams=n_streams, mask_padding=mask_padding,
                    causal=causal)
    rows = []
    for epoch in range(epochs):
        last = kept = None
        for batch in batches:
            if reserve_S and eng._shape is None:
                S0, B0 = batch["text"].shape[:2]
                eng.reserve(max(reserve_S, S0), B0)
            eng.iteration(batch)
            if log:
                last = eng.loss_dict()
                log(epoch, last)
            else:
                # nobody reads this batch's losses on the host: keep a device-side copy (the next iteration overwrites
                # eng.losses) and read the last one once, after the epoch — the host runs ahead of the GPU meanwhile
                eng.synchronize()
                kept = eng.losses.clone()
        if kept is not None:
            last = {"%s_%s_loss" % (who, kind): x for (kind, who, _), x in zip(eng.schedule, kept.tolist())}
        if last is not None:
            rows.append(dict(epoch=epoch, **{c: last[c] for c in LOSS_COLUMNS}))
    return rows


# ================================================================================================
# Phase 2: GAN_FFN classifier step      (/root/reference/model.py:1434-1462, train_IEMOCAP.py:103-197,653-661)
# ================================================================================================
CLASS_WEIGHTS = [1.2, 0.60072, 0.38066, 0.94019, 0.67924, 0.34332]   # train_IEMOCAP.py:653


def _module_generators(module, lr, weight_decay):
    """the three generators of a classifier module as NetStates under its Adam(0.9, 0.999, L2), in the order the module runs them
    (model.py:1441-1443, 1521-1523)"""
    return {k: NetState(getattr(module, k + "_generator"), lr, (0.9, 0.999), weight_decay)
            for k in ("acoustic", "visual", "text")}


def _generator_bwd(eng, k, d_out, adds):
    """one generator's backward from d_out, its all-reduce and its Adam, on the current stream with the workspace eng.ws"""
    net = eng.G[k]
    net.grad.zero_()
    cb, finish = eng._make_reducer(net)
    eng._net_bwd(net, eng.pass_G[k], d_out, True, adds, True, cb)
    finish(("G", k))


class Phase2Engine(_NetRunner):
    """One step of train_or_eval_model on GAN_FFN: log_softmax(fc(G_a(a) + G_v(v) + G_t(t))), MaskedNLLLoss with
    class weights, backward through the three generators, Adam(lr, weight_decay=l2) on everything.
    The reference re-creates a LambdaLR every batch, which pins the effective lr to its base value.
    mask_padding (default False: the reference passes no mask) is an extension: the three generators' self-attention sees only the
    first umask.sum(1) utterances of every dialogue (ganffn_encoder_fwd_len / _bwd_len), so a dialogue's prediction does not depend
    on how far its batch is padded.  umask must then be a prefix mask.  False issues exactly the calls it always did.
    causal (default False: the reference's generators are bidirectional) is an extension too: in the three generators utterance i
    attends to utterances j <= i only (ganffn_encoder_fwd_mask / _bwd_mask with GANFFN_ATTN_CAUSAL), so log_prob[t] is a function
    of utterances 0 .. t — a classifier that can run while the dialogue is spoken.  It composes with mask_padding and alone needs
    no lengths.  False issues exactly the calls it always did."""

    def __init__(self, ffn_module, lr=1e-4, weight_decay=0.008, class_weights=CLASS_WEIGHTS, process_group=None,
                 n_buckets=3, mask_padding=False, causal=False):
        self.mask_padding = bool(mask_padding)
        self._causal = self.causal = bool(causal)
        self.module = ffn_module
        self.G = _module_generators(ffn_module, lr, weight_decay)
        self._init_common(next(iter(self.G.values())).slab.device, process_group, n_buckets, self.G.items())
        self.n_classes = ffn_module.fc.weight.shape[0]
        dev = self.dev
        # fc (100 -> n_classes) parameters as one small slab [weight | bias], 16-byte aligned pieces
        self.fc_w, self.fc_b = ffn_module.fc.weight, ffn_module.fc.bias
        fc = self.fc = _ParamSlab([self.fc_w, self.fc_b], dev)
        self.fc_slab, self.fc_grad, self.fc_m, self.fc_v, self.fc_step = fc.slab, fc.grad, fc.exp_avg, fc.exp_avg_sq, fc.step
        self.fc_off_b, self.fc_total = fc.offs[1], fc.total
        self.lr, self.wd = lr, weight_decay
        self.class_w = torch.tensor(class_weights, device=dev, dtype=torch.float32) if class_weights is not None else None
        self.loss = torch.zeros(1, device=dev)

    def _prepare2(self, S, B):
        fit = self._fit(S, B)
        if fit == "same":
            return
        C_ = self.n_classes
        if fit == "grow":
            cS, cB, dev = self._alloc_S, self._alloc_B, self.dev
            self.pass_G = {k: _Pass(n, cS, cB, dev, True) for k, n in self.G.items()}
            n_ws = max(p.n_ws for p in self.pass_G.values())
            f32 = dict(device=dev, dtype=torch.float32)
            self.ws = torch.empty(n_ws, **f32)
            self._flat = dict(fusion=torch.empty(cS * cB * 100, **f32), logits=torch.empty(cS * cB * C_, **f32),
                              log_prob=torch.empty(cS * cB * C_, **f32), dlogits=torch.empty(cS * cB * C_, **f32),
                              d_fusion=torch.empty(cS * cB * 100, **f32))
            self.ws2 = torch.zeros(4, **f32)
        for p_ in self.pass_G.values():
            p_.resize(S, B)
        f = self._flat
        self.fusion = f["fusion"][:S * B * 100].view(S, B, 100)
        self.logits = f["logits"][:S * B * C_].view(S, B, C_)
        self.log_prob = f["log_prob"][:S * B * C_].view(S, B, C_)
        self.dlogits = f["dlogits"][:S * B * C_].view(S, B, C_)
        self.d_fusion = f["d_fusion"][:S * B * 100].view(S, B, 100)

    def step(self, batch, train=True):
        """batch: text/visual/acoustic (S,B,.), umask (B,S) float, label (B,S) int64.  Returns (loss tensor, log_prob).
        train=False: forward + loss only (model.eval())."""
        S, B = batch["text"].shape[:2]
        self._prepare2(S, B)
        self._check_slabs()
        if not self.fc.in_place():
            raise RuntimeError("GAN_FFN.fc was re-allocated after the engine was built: build Phase2Engine after the last .to()")
        T, C_ = S * B, self.n_classes
        self._adds = 0
        self._base_add = self.rng.next_add(8)      # 3 generators x (encoder, head): one block from the device allocator
        if self.mask_padding and ops._CHECK_QMASK:
            ops.check_prefix_mask(batch["umask"], "Phase2Engine")
        self._key_len = ops.key_lengths_from_umask(batch["umask"]) if self.mask_padding else None   # on the device: no host read
        adds = {}
        for k in ("acoustic", "visual", "text"):                    # model.py:1441-1443
            adds[k] = self._net_fwd(self.G[k], self.pass_G[k], batch[k], train=train, save=train)
        ops.add3_raw(self.pass_G["acoustic"].out, self.pass_G["visual"].out, self.pass_G["text"].out, self.fusion, T * 100)
        ops.linear_fwd_raw(self.fusion, self.fc_w, self.fc_b, self.logits, T, 100, C_)          # model.py:1448
        ops.logsoftmax_nll_raw(self.logits, batch["label"], batch["umask"], self.class_w, self.log_prob, self.loss,
                               self.dlogits if train else None, self.ws2, S, B, C_)                # model.py:1449, :74-81
        if train:
            self.fc_grad.zero_()
            ops.linear_bwd_raw(self.dlogits, self.fusion, self.fc_w, self.d_fusion, self.fc_grad[:self.fc_w.numel()],
                               self.fc_grad[self.fc_off_b:], T, 100, C_, self.ws)
            for k in ("acoustic", "visual", "text"):
                _generator_bwd(self, k, self.d_fusion, adds[k])
            self.fc.all_reduce(self.pg)
            self.fc.adam(self.lr, self.wd, self.world)
        assert self._adds <= 8, self._adds
        return self.loss, self.log_prob


# ================================================================================================
# Configuration 5: GAN_FFN_DialogueRNN classifier step     (/root/reference/train_IEMOCAP_DialogueRNN.py:705-760,
#                                                          model.py:975-1062, 1465-1528)
# ================================================================================================
SITE_JOIN_F, SITE_JOIN_B, SITE_HIDDEN = 5, 6, 7       # dropout sites of the head (the recurrence uses 8..14, the encoders 16+)


_MAX_DIALOGUES_HINT = " (max_dialogues: the constructor takes up to %d)" % ops.MAX_DIALOGUES


def _check_max_dialogues(who, n):
    """a step runner's dialogue capacity: 32 (the default: one tile of the recurrences' products) .. ops.MAX_DIALOGUES"""
    n = int(n)
    if not 32 <= n <= ops.MAX_DIALOGUES:
        raise ValueError("%s: max_dialogues = %d outside [32, %d] (ops.MAX_DIALOGUES: the most dialogues a native call of the "
                         "recurrence takes) — split the batch, or run the module path, which chunks by itself"
                         % (who, n, ops.MAX_DIALOGUES))
    return n


class DrnnEngine(_NetRunner):
    """One train / eval step of GAN_FFN_DialogueRNN on the C ABI, no autograd graph: the three generators (n_streams = 3
    runs their forward and backward passes on three HIP streams chosen by _side_streams with its own _tune_slot as probe;
    measured NOT faster than one stream on this workload — 15.0-16.5 against 14.9-15.0 ms per step: kernels of different
    streams do not run side by side, only the dead time between launches overlaps, and the run-to-run
    spread grows — so one stream is the default), fusion = their sum, BiModel's two
    DialogueRNN directions through one chain of launches (ops.drnn_fwd_raw / drnn_bwd_raw), the matching attention
    (ganffn_general2_attention_*), linear + ReLU + dropout, the class head, MaskedNLLLoss with class weights, and Adam
    (lr, L2-coupled weight decay; train_IEMOCAP_DialogueRNN.py:746) on flat slabs: one fused launch per generator and one
    for the whole head.  Data-parallel: the generators' gradients go through the bucketed GradReducer (all-reduce of a
    bucket overlaps the rest of that generator's backward, Adam per bucket), the head's slab is one more bucket.
    Supports every context attention type of the reference script's --attention (general — the trained configuration —,
    simple (passed on as its own type), dot, general2, concat), 1 to ops.DRNN_MAX_PARTIES parties (qmask (S, B, P); the slab
    does not depend on P), with or without listener state (--active-listener: the 4 l_cell tensors per direction at the end
    of the head slab).  Which entry points of the recurrence a step reaches: ops.drnn_family.  general keeps the slab layout
    it always had; the other types have their attention tensors in the cell block (ops.DRNN_ATT_KEYS: named_parameters
    order).  The module path (model.GAN_FFN_DialogueRNN.forward under autograd) stays available for what the kernels cannot
    run (D_g != D_p, D_g > 512, dot with D_m != D_g, concat D_a limits).
    max_dialogues (32 .. ops.MAX_DIALOGUES; default 32): the most dialogues a step takes.  It is a capacity, not a switch: the
    family is decided from the batch's own B (more than 32 dialogues: the same step with the dialogues in tiles of 32 inside
    every launch).
    mask_padding (default False: the reference passes no mask) is an extension: the generators' self-attention sees only the first
    umask.sum(1) utterances of every dialogue — the lengths tensor the recurrence already uses, so the step has no launch more —
    and with that no part of the step lets padding reach a real utterance.  False issues exactly the calls it always did.
    A causal net (GAN_FFN_DialogueRNN(causal=True): net.causal, read from the module — the head's structure is the module's, so
    there is no constructor argument; absent means False) is a classifier that never looks ahead, and the step follows it: the
    generators run forward and backward under the causal flag (with the key lengths when mask_padding), there is ONE recurrence
    direction (ndir = 1: no ganffn_seq_reverse, no reversed speaker indices), the join is a dropout of e_f alone (ganffn_dropout
    at SITE_JOIN_F, forward and on the gradient; skipped in eval), the head is D_e wide (transform D_e -> D_e, the CAUSAL
    general2 attention through ganffn_general2_attention_*_mask, linear D_e -> D_h) and d_fusion is the recurrence's dU.  The
    head slab holds one cell's tensors, the six head tensors, then the one cell's listener tensors; the step's block of RNG
    offsets keeps its layout.  A bidirectional net issues exactly the calls it always did."""

    def __init__(self, net, lr=1e-4, weight_decay=1e-5, class_weights=CLASS_WEIGHTS, process_group=None, n_buckets=3,
                 n_streams=1, max_dialogues=32, mask_padding=False):
        from . import dialogue_rnn as DR
        self.mask_padding = bool(mask_padding)
        self.max_dialogues = _check_max_dialogues("DrnnEngine", max_dialogues)
        self.module = net
        bm = net.bi_model
        self._causal = self.causal = bool(getattr(net, "causal", False))
        self.ndir = 1 if self.causal else 2                  # directions of the recurrence = cells on the head slab
        cells = [bm.dialog_rnn_f.dialogue_cell] + ([] if self.causal else [bm.dialog_rnn_r.dialogue_cell])
        cf = cells[0]
        if cf.D_g != cf.D_p or cf.D_g > 512 or cf.D_g % 4 or not ops.drnn_att_limits_hold(cf):
            raise ValueError("DrnnEngine runs every context attention type (general, simple, dot, general2, concat) within the "
                             "recurrence kernels' limits: D_g = D_p <= 512 (multiples of 4), dot only with D_m = D_g, concat "
                             "only with D_a a multiple of 4 and <= 512; got %s attention, D_m = %d, D_g = %d, D_p = %d — use "
                             "the module path for the rest" % (ops.drnn_att_type(cf), cf.D_m, cf.D_g, cf.D_p))
        self.listener = bool(cf.listener_state)
        self.att = ops.drnn_att_type(cf)
        self.att_keys = ops.DRNN_ATT_KEYS[self.att]
        self.ncell = 12 + len(self.att_keys)                 # tensors per cell in the slab (13 for general: layout unchanged)
        self.acfg = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[self.att],
                                 int(cf.attention.transform.weight.shape[0]) if self.att == "concat" else 0)
        self.G = _module_generators(net, lr, weight_decay)
        self._init_common(next(iter(self.G.values())).slab.device, process_group, n_buckets, self.G.items())
        dev = self.dev
        self.lr, self.wd = lr, weight_decay
        self.Dm, self.H, self.He, self.Dh2 = cf.D_m, cf.D_g, cf.D_e, bm.linear.weight.shape[0]
        self.D2 = self.ndir * cf.D_e                         # width of the head's rows (the joined emotions)
        self.n_classes = bm.smax_fc.weight.shape[0]
        self.p_rec, self.p_join, self.p_hid = float(cf.dropout.p), float(bm.dropout_rec.p), float(bm.dropout.p)
        # ---- head parameters -> one slab (views keep the module's parameters alive on it)
        plist = []
        for cell in cells:
            sd = dict(cell.named_parameters())
            plist += [sd[k] for k in ops.DRNN_KEYS[:12] + self.att_keys]
        plist += [bm.matchatt.transform.weight, bm.matchatt.transform.bias, bm.linear.weight, bm.linear.bias,
                  bm.smax_fc.weight, bm.smax_fc.bias]
        if self.listener:                    # behind the head tensors: the listener-free slab layout does not move
            for cell in cells:
                sd = dict(cell.named_parameters())
                plist += [sd[k] for k in ops.DRNN_LISTENER_KEYS]
        head = self.head = _ParamSlab(plist, dev)
        self.h_slab, self.h_grad, self.h_m, self.h_v, self.h_step = head.slab, head.grad, head.exp_avg, head.exp_avg_sq, head.step
        self._hparams, self._hoffs, self.h_total, self._hp = head.params, head.offs, head.total, head.view
        self.class_w = torch.tensor(class_weights, device=dev, dtype=torch.float32) if class_weights is not None else None
        self.n_streams = max(1, min(3, n_streams))
        if process_group is not None:
            self.n_streams = 1           # (one communicator: its in-line collectives must not run on several streams at once)
        self.streams = None                                  # (n_streams > 1: chosen in _prepare5, once the buffers exist)
        self._tune_x = (None, None)                          # (shape, inputs) of _tune_slot's probe work
        self.loss = torch.zeros(1, device=dev)
        self._alloc_P = 0                                    # parties the recurrence's buffers are sized for

    def _check_SB(self, S, B):
        if B > self.max_dialogues or S > 112:
            raise ValueError("DrnnEngine: at most %d dialogues%s of at most 112 utterances per step (the recurrence's tile and the "
                             "attention kernels' sequence limit); got S = %d, B = %d — split the batch, or run the module path "
                             "(model.GAN_FFN_DialogueRNN under autograd, which chunks by itself)"
                             % (self.max_dialogues, _MAX_DIALOGUES_HINT if self.max_dialogues < ops.MAX_DIALOGUES else "", S, B))

    def _prepare5(self, S, B, P=2):
        fit = self._fit(S, B, P, grow=P > self._alloc_P)
        if fit == "same":
            return
        if fit == "grow":
            cS, cB, dev = self._alloc_S, self._alloc_B, self.dev
            cP = self._alloc_P = max(self._alloc_P, P)
            self.pass_G = {k: _Pass(n, cS, cB, dev, True) for k, n in self.G.items()}
            f32 = dict(device=dev, dtype=torch.float32)
            self.ws3 = {k: torch.empty(p_.n_ws, **f32) for k, p_ in self.pass_G.items()}     # one workspace per generator stream
            cfgc = _lib.DrnnCfg(cS, cB, self.Dm, self.H, self.He, self.p_rec, 1)
            lib = _lib.load()
            # (the capacity's family: the layouts are the same functions of B in every family, and the recurrence's buffers grow
            # with the party count — sized for the widest batch so far)
            n_saved, n_ws = ops.drnn_floats(cfgc, self.acfg, self.listener, cP)
            T, D2, Cn = cS * cB, self.D2, self.n_classes
            z = lambda n: torch.empty(n, **f32)
            zb = (lambda n: None) if self.causal else z      # the second direction's buffers: a causal net has none
            self._f = dict(fusion=z(T * self.Dm), rev_U=zb(T * self.Dm), e_f=z(T * self.He), e_b=zb(T * self.He),
                           alpha_f=z(cB * cS * cS), alpha_b=zb(cB * cS * cS), emotions=z(T * D2), xq=z(T * D2), att=z(T * D2),
                           alpha2=z(cB * cS * cS), tanh_s=z(cB * cS * cS), du=z(cB * cS * cS), hidden=z(T * self.Dh2),
                           logits=z(T * Cn), log_prob=z(T * Cn), dlogits=z(T * Cn), d_hidden=z(T * self.Dh2), d_att=z(T * D2),
                           d_xq=z(T * D2), d_mem=z(T * D2), d_em=z(T * D2), d_e_f=z(T * self.He), d_e_b=zb(T * self.He),
                           dU_f=z(T * self.Dm), dU_b=zb(T * self.Dm), saved_f=z(n_saved), saved_b=zb(n_saved), ws_f=z(n_ws),
                           ws_b=zb(n_ws), lin_ws=z(int(lib.ganffn_linear_bwd_workspace_floats(T, D2, D2)) + 64))
            self.ws2 = torch.zeros(4, **f32)
        for p_ in self.pass_G.values():
            p_.resize(S, B)
        self.cfg_train = _lib.DrnnCfg(S, B, self.Dm, self.H, self.He, self.p_rec, 1)
        self.cfg_eval = _lib.DrnnCfg(S, B, self.Dm, self.H, self.He, self.p_rec, 0)
        if self.n_streams > 1 and self.streams is None:
            self.streams = list(_side_streams(self.dev, [0, 0, 0], self._tune_streams, S * B))
            self._tune_x = (None, None)

    def _tune_slot(self, i):
        k = ("acoustic", "visual", "text")[i % 3]
        if self._tune_x[0] != self._shape:
            S, B = self._shape[:2]
            self._tune_x = (self._shape, {m: torch.zeros(S, B, self.G[m].E, device=self.dev) for m in self.G})
        self.ws = self.ws3[k]
        if self.mask_padding and (self._key_len is None or self._key_len.numel() != self._shape[1]):
            self._key_len = torch.full((self._shape[1],), self._shape[0], device=self.dev, dtype=torch.int32)     # the probe: full lengths
        # (save=True: these pass buffers and their workspace were sized for the saving mode; the next real forward overwrites)
        self._net_fwd(self.G[k], self.pass_G[k], self._tune_x[1][k], train=False, save=True, adds=(0, 1))

    # ------------------------------------------------------------------------------------------
    # pointer structs of the ndir directions over the head slab (grad: over its gradient slab), built by the ops helpers
    def _drnn_ptrs(self, grad):
        # (the first ncell fields; other types than general: att_w stays NULL)
        return ops._ptr_structs(_lib.DrnnPtrs, [[self._hp(self.ncell * z + j, grad) for j in range(self.ncell)]
                                                for z in range(self.ndir)])

    def _drnn_att_ptrs(self, grad):
        n = len(self.att_keys)
        return ops._ptr_structs(_lib.DrnnAttPtrs, [[self._hp(self.ncell * z + 12 + i, grad) for i in range(n)]
                                                   for z in range(self.ndir)], lambda a, _: ops._att_ptrs(self.att, a))

    def _drnn_listener_ptrs(self, grad):
        return ops._ptr_structs(_lib.DrnnListenerPtrs, [[self._hp(self.ndir * self.ncell + 6 + 4 * z + j, grad) for j in range(4)]
                                                        for z in range(self.ndir)])

    def step(self, batch, train=True):
        """batch: acoustic/visual/text (S,B,.), qmask (S,B,P) one-hot (zero rows on padding; 1 <= P <= ops.DRNN_MAX_PARTIES),
        umask (B,S), label (B,S) int64.  Returns (loss tensor, log_prob (S,B,C)).  train=False: forward + loss only
        (model.eval())."""
        S, B = batch["text"].shape[:2]
        P = batch["qmask"].size(2)
        if not 1 <= P <= ops.DRNN_MAX_PARTIES:
            raise ValueError("DrnnEngine: qmask has %d parties; the recurrence kernels take 1 to %d (ops.DRNN_MAX_PARTIES) — run "
                             "the module path (model.GAN_FFN_DialogueRNN under autograd) for more" % (P, ops.DRNN_MAX_PARTIES))
        self._prepare5(S, B, P)
        if self.streams is None:
            return self._step(batch, train)
        # n_streams = 3: the WHOLE step runs on the tuned streams — the visual generator's stream carries the recurrence and
        # the head as well, the two 100-wide generators run beside it — and the caller's stream only waits at both ends
        # (round 3 ran the recurrence on the caller's stream, a fourth stream the tuner had not chosen).  Section timing
        # (tools/lab/drnn_sections.py, gpurun_out/r4_drnn_sections*.txt): the three generators' forward 3.75 -> 3.3 ms and
        # backward + Adam 5.69 -> 4.9 ms on three streams, but the recurrence + head — a chain of ~400 latency-sized launches —
        # 5.84 -> 6.3-7.3 ms as soon as the process has several active hardware queues, whichever stream it runs on:
        # 14.45-15.6 ms against 14.8-15.3 on one stream depending on the box.  One stream stays the default.
        cur = torch.cuda.current_stream()
        main = self.streams[1]
        main.wait_stream(cur)
        for t_ in batch.values():
            if torch.is_tensor(t_) and t_.is_cuda:
                t_.record_stream(main)
        with torch.cuda.stream(main):
            out = self._step(batch, train)
        cur.wait_stream(main)
        return out

    def _step(self, batch, train=True):
        S, B = batch["text"].shape[:2]
        self._check_slabs()
        if not self.head.in_place():
            raise RuntimeError("the DialogueRNN head was re-allocated after the engine was built: build DrnnEngine after the last .to()")
        P, st_ = ops._ptr, ops._stream
        T, Dm, He, D2, Cn = S * B, self.Dm, self.He, self.D2, self.n_classes
        f, nd, causal = self._f, self.ndir, self.causal
        self._adds = 0
        self._base_add = self.rng.next_add(10)          # 3 generators x (encoder, head), the recurrence, the head's dropouts
        a_rec, a_head = self._base_add + 6, self._base_add + 7
        rng = self.rng.state
        umask, qmask = batch["umask"], batch["qmask"]
        if ops._CHECK_QMASK:
            # GANFFN_CHECK_QMASK=1 (one host sync per batch): the gate kernels use argmax / max of a qmask row and the lengths
            # umask.sum(1) — a soft or multi-hot speaker row or a mask with holes would silently differ from the reference
            row = qmask.sum(2)
            if not bool((((row == 1) & (qmask.max(2).values == 1)) | (row == 0)).all()):
                raise ValueError("DrnnEngine: qmask rows must be one-hot (or all zero on padding)")
            ops.check_prefix_mask(umask, "DrnnEngine")
        # per-batch index data (tiny): dialogue lengths, speaker index / value per step, in both directions
        lens = umask.sum(1).to(torch.int32)
        self._key_len = lens if self.mask_padding else None
        spk_f = torch.argmax(qmask, 2).to(torch.int32).contiguous()
        mval_f = qmask.max(2).values.contiguous()
        if not causal:
            t_idx = torch.arange(S, device=self.dev).unsqueeze(1)
            src = (lens.to(torch.long).unsqueeze(0) - 1 - t_idx).clamp(min=0)
            valid = (t_idx < lens.unsqueeze(0))
            spk_b = (spk_f.gather(0, src) * valid).to(torch.int32).contiguous()
            mval_b = (mval_f.gather(0, src) * valid).contiguous()

        # ---- three generators, concurrently
        keys = ("acoustic", "visual", "text")                        # model.py:1521-1523
        adds = {}
        cur = torch.cuda.current_stream()
        if self.streams is not None:
            fork = torch.cuda.Event()
            fork.record(cur)
        for i, k in enumerate(keys):
            self.ws = self.ws3[k]
            if self.streams is not None and self.streams[i].cuda_stream != cur.cuda_stream:
                self.streams[i].wait_event(fork)
                if batch[k].is_cuda:
                    batch[k].record_stream(self.streams[i])      # the caller may drop the batch while this stream still reads it
                if self._key_len is not None:
                    self._key_len.record_stream(self.streams[i])
                with torch.cuda.stream(self.streams[i]):
                    adds[k] = self._net_fwd(self.G[k], self.pass_G[k], batch[k], train=train, save=train)
            else:
                adds[k] = self._net_fwd(self.G[k], self.pass_G[k], batch[k], train=train, save=train)
        if self.streams is not None:
            for s_ in self.streams:
                if s_.cuda_stream != cur.cuda_stream:
                    cur.wait_stream(s_)
        st = st_()
        ops.add3_raw(self.pass_G["acoustic"].out, self.pass_G["visual"].out, self.pass_G["text"].out, f["fusion"], T * Dm)
        if not causal:
            _lib.call("ganffn_seq_reverse", P(f["fusion"]), P(lens), P(f["rev_U"]), S, B, Dm, 0, st)
        # ---- the recurrence, both directions (a causal net: the forward one alone)
        cfg = self.cfg_train if train else self.cfg_eval
        arr = lambda ts: (C.c_void_p * nd)(*[t.data_ptr() for t in ts[:nd]])
        U_, spk_, mval_ = arr([f["fusion"], f["rev_U"]]), arr([spk_f, None if causal else spk_b]), arr([mval_f, None if causal else mval_b])
        e_, al_, sv_, ws_ = arr([f["e_f"], f["e_b"]]), arr([f["alpha_f"], f["alpha_b"]]), arr([f["saved_f"], f["saved_b"]]), arr([f["ws_f"], f["ws_b"]])
        Pp, APp = self._drnn_ptrs(False), self._drnn_att_ptrs(False)
        LPp = self._drnn_listener_ptrs(False) if self.listener else None
        parties = self._shape[2]
        ops.drnn_fwd_raw(cfg, self.acfg, parties, nd, U_, spk_, mval_, Pp, LPp, APp, e_, al_, sv_, ws_, P(rng), a_rec)
        # ---- head: emotions -> matching attention -> linear/relu/dropout -> classes -> loss
        tr, a_flags = 1 if train else 0, ops.ATTN_CAUSAL if causal else None
        w_t, b_t, w_l, b_l, w_s, b_s = (self._hp(nd * self.ncell + j) for j in range(6))
        if causal:
            # the join of one direction is dropout_rec on e_f alone (SITE_JOIN_F); eval: the emotions are e_f itself
            em = f["emotions"] if train else f["e_f"]
            if train:
                ops.dropout_raw(f["e_f"], em, T, He, self.p_join, SITE_JOIN_F, rng, a_head)
        else:
            em = f["emotions"]
            _lib.call("ganffn_drnn_join_fwd", P(f["e_f"]), P(f["e_b"]), P(lens), P(em), S, B, He, C.c_float(self.p_join),
                      C.c_uint32(SITE_JOIN_F), C.c_uint32(SITE_JOIN_B), P(rng), C.c_uint64(a_head), tr, st)
        ops.linear_fwd_raw(em, w_t, b_t, f["xq"], T, D2, D2)
        ops.general2_attention_fwd_raw(f["xq"], em, umask, f["att"], f["alpha2"], f["tanh_s"], S, B, D2, a_flags)
        ops.linear1_fwd_raw(f["att"], w_l, b_l, f["hidden"], T, D2, self.Dh2, self.p_hid, SITE_HIDDEN, rng, a_head, train)
        ops.linear_fwd_raw(f["hidden"], w_s, b_s, f["logits"], T, self.Dh2, Cn)
        log_prob = f["log_prob"][:T * Cn].view(S, B, Cn)
        ops.logsoftmax_nll_raw(f["logits"], batch["label"], umask, self.class_w, log_prob, self.loss,
                               f["dlogits"] if train else None, self.ws2, S, B, Cn)
        if not train:
            return self.loss, log_prob
        # ---- backward through the head
        self.h_grad.zero_()
        g_t, gb_t, g_l, gb_l, g_s, gb_s = (self._hp(nd * self.ncell + j, True) for j in range(6))
        ops.linear_bwd_raw(f["dlogits"], f["hidden"], w_s, f["d_hidden"], g_s, gb_s, T, self.Dh2, Cn, f["lin_ws"])
        mscale = 1.0 / (1.0 - self.p_hid) if self.p_hid > 0 else 1.0
        _lib.call("ganffn_mask_pos_inplace", P(f["d_hidden"]), P(f["hidden"]), C.c_float(mscale), C.c_int64(T * self.Dh2), st)
        ops.linear_bwd_raw(f["d_hidden"], f["att"], w_l, f["d_att"], g_l, gb_l, T, D2, self.Dh2, f["lin_ws"])
        ops.general2_attention_bwd_raw(f["d_att"], f["xq"], em, umask, f["alpha2"], f["tanh_s"], f["du"], f["d_xq"], f["d_mem"], S, B, D2,
                                       a_flags)
        ops.linear_bwd_raw(f["d_xq"], em, w_t, f["d_em"], g_t, gb_t, T, D2, D2, f["lin_ws"])
        f["d_em"][:T * D2].add_(f["d_mem"][:T * D2])          # memory path of the attention + its transform(mem) path
        if causal:
            ops.dropout_raw(f["d_em"], f["d_e_f"], T, He, self.p_join, SITE_JOIN_F, rng, a_head)
        else:
            _lib.call("ganffn_drnn_join_bwd", P(f["d_em"]), P(lens), P(f["d_e_f"]), P(f["d_e_b"]), S, B, He, C.c_float(self.p_join),
                      C.c_uint32(SITE_JOIN_F), C.c_uint32(SITE_JOIN_B), P(rng), C.c_uint64(a_head), tr, st)
        # ---- the recurrence backward (weight gradients accumulate into the zeroed head slab)
        Gp = self._drnn_ptrs(True)
        de_, dU_ = arr([f["d_e_f"], f["d_e_b"]]), arr([f["dU_f"], f["dU_b"]])
        ops.drnn_bwd_raw(cfg, self.acfg, parties, nd, de_, U_, spk_, mval_, Pp, LPp, APp, Gp,
                         self._drnn_listener_ptrs(True) if self.listener else None, self._drnn_att_ptrs(True), dU_, al_, sv_, ws_,
                         P(rng), a_rec)
        # d fusion = dU_f + reverse(dU_b); a causal net: dU_f itself
        if not causal:
            _lib.call("ganffn_seq_reverse", P(f["dU_b"]), P(lens), P(f["dU_f"]), S, B, Dm, 1, st)
        d_fusion = f["dU_f"][:T * Dm].view(S, B, Dm)
        # ---- head optimizer step (its all-reduce, when data-parallel, runs beside the generators' backward)
        # (in-line mode: on this stream — a communicator never carries two collectives at once, and the generators' all-reduces
        # below use the same one; bucket mode: finished after the generators' backward)
        red_h = self.head.all_reduce(self.pg, wait=False)
        # ---- three generator backward passes + Adam, concurrently
        if self.streams is not None:
            fork = torch.cuda.Event()
            fork.record(cur)
        for i, k in enumerate(keys):
            self.ws = self.ws3[k]
            if self.streams is not None and self.streams[i].cuda_stream != cur.cuda_stream:
                self.streams[i].wait_event(fork)
                with torch.cuda.stream(self.streams[i]):
                    _generator_bwd(self, k, d_fusion, adds[k])
            else:
                _generator_bwd(self, k, d_fusion, adds[k])
        if red_h is not None:
            red_h.finish()
        self.head.adam(self.lr, self.wd, self.world)
        if self.streams is not None:
            for s_ in self.streams:
                if s_.cuda_stream != cur.cuda_stream:
                    cur.wait_stream(s_)
        assert self._adds <= 6, self._adds
        return self.loss, log_prob


# ================================================================================================
# MELD: MELDLSTMModel classifier step     (/root/reference/train_MELD.py:50-104,147-157, model.py:520-562)
# ================================================================================================
class MeldEngine(_Runner):
    """One train / eval step of MELDLSTMModel (the att2 = True branch train_MELD.py:71 runs) on the C ABI, no autograd graph:
    the 4-layer bidirectional LSTM with its inter-layer dropout as ONE library call (ganffn_lstm_stack_fwd / _bwd), matchatt's
    transform (ganffn_linear_*), the masked general2 attention (ganffn_general2_attention_*), hardswish(emotions + hardswish(att))
    and smax_fc as one launch each way (ganffn_meld_head_*), log-softmax + MaskedNLLLoss — without class weights by default, as
    train_MELD.py:154 — and Adam (lr 3e-4, L2 1e-4: train_MELD.py:111-112,155-157) as ONE fused launch over one parameter slab:
    the LSTM's 32 tensors in named_parameters() order, matchatt.transform.{weight, bias}, smax_fc.{weight, bias}.
    `linear.{weight, bias}` serve the att2 = False branch only: their .grad is None in the reference, torch.optim.Adam skips such
    parameters entirely (no weight decay either), so they stay off the slab and are never touched.
    Limits (ValueError; MELDLSTMModel under autograd — the module path — runs the rest): at most max_dialogues dialogues (32 ..
    ops.MAX_DIALOGUES, default 32: a capacity — up to 32 dialogues run ganffn_lstm_stack_*, more ganffn_lstm_stack_batch_*, decided
    from B alone) of at most 128 utterances per step, 2 D_e <= 1024, D_m and D_e multiples of 4, at most 16 classes.
    packed = True (default False; an extension the reference does not have, MELDLSTMModel(packed=True)'s step): the LSTM runs on
    packed sequences — lengths = umask.sum(1) as int32, derived on the device every step (umask must be a prefix mask), through
    ganffn_lstm_stack_packed_* for any B <= max_dialogues: the same launches; everything else in the step is unchanged.
    A model built with causal=True (MELDLSTMModel(causal=True); an extension the reference does not have; read from the model,
    and refused when it contradicts lstm.bidirectional) steps the classifier that never looks ahead: one direction (D = D_e
    instead of 2 D_e everywhere above), the LSTM's 4 L tensors on the slab, pointer arrays [L][1], the same ops.lstm_stack_*_raw
    calls with ndir=1 (ops.lstm_family: ganffn_unilstm_stack_* for any B <= max_dialogues, lengths or NULL) and the attention through
    ganffn_general2_attention_fwd_mask / _bwd_mask with GANFFN_ATTN_CAUSAL; the rest of the step is the same calls.  Its limits:
    D_e <= 1024, D_m and D_e multiples of 4, smax_fc and matchatt D_e wide.  A default model issues the calls it always did.
    Data-parallel over dialogues like Phase2Engine: the gradient slab is all-reduced in-line on the step's stream (through
    GradReducer under GANFFN_DP_MODE=buckets), Adam divides by the world size."""

    def __init__(self, model, lr=3e-4, weight_decay=1e-4, class_weights=None, process_group=None, max_dialogues=32, packed=False):
        self.max_dialogues = _check_max_dialogues("MeldEngine", max_dialogues)
        self.packed = bool(packed)
        self.module = model
        lstm = model.lstm
        self.causal = bool(getattr(model, "causal", False))
        if hasattr(model, "causal") and self.causal == bool(lstm.bidirectional):
            raise ValueError("MeldEngine: model.causal = %s contradicts lstm.bidirectional = %s (MELDLSTMModel(causal=True) builds a "
                             "forward-only LSTM, the default a bidirectional one) — run the module path (MELDLSTMModel under "
                             "autograd) for anything else" % (self.causal, bool(lstm.bidirectional)))
        if not (lstm.bidirectional != self.causal and not lstm.batch_first and lstm.proj_size == 0 and lstm.bias):
            raise ValueError("MeldEngine: MELDLSTMModel's LSTM configuration only (bidirectional, sequence-first, biases, no "
                             "projection) — run the module path for anything else")
        self.Dm, self.He, self.L = int(lstm.input_size), int(lstm.hidden_size), int(lstm.num_layers)
        self.ndir = 1 if self.causal else 2
        self.D2 = self.ndir * self.He             # the width of the LSTM's output: 2 D_e, or D_e for the causal model
        self.n_classes = int(model.smax_fc.weight.shape[0])
        self.p_lstm = float(lstm.dropout)
        if (self.Dm % 4 or self.He % 4 or self.D2 > 1024 or self.n_classes > 16 or model.smax_fc.weight.shape[1] != self.D2
                or model.matchatt.att_type != "general2" or tuple(model.matchatt.transform.weight.shape) != (self.D2, self.D2)):
            if self.causal:
                raise ValueError("MeldEngine: a causal model's D_m and D_e must be multiples of 4, D_e <= 1024 (the general2 attention "
                                 "kernel), at most 16 classes, smax_fc and matchatt D_e wide; got D_m = %d, D_e = %d, %d classes, "
                                 "smax_fc over %d — use the module path (MELDLSTMModel under autograd) for the rest"
                                 % (self.Dm, self.He, self.n_classes, model.smax_fc.weight.shape[1]))
            raise ValueError("MeldEngine: D_m and D_e must be multiples of 4, 2 D_e <= 1024 (the general2 attention kernel), at most "
                             "16 classes, smax_fc and matchatt 2 D_e wide; got D_m = %d, D_e = %d, %d classes, smax_fc over %d — use "
                             "the module path (MELDLSTMModel under autograd) for the rest"
                             % (self.Dm, self.He, self.n_classes, model.smax_fc.weight.shape[1]))
        names = dict(lstm.named_parameters())
        plist = [names[k] for k in names]                     # weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, *_l0_reverse, ...
        assert len(plist) == 4 * self.ndir * self.L and (self.causal or list(names)[4] == "weight_ih_l0_reverse"), list(names)[:8]
        plist += [model.matchatt.transform.weight, model.matchatt.transform.bias, model.smax_fc.weight, model.smax_fc.bias]
        self._init_common(plist[0].device, process_group, 1)
        dev = self.dev
        assert dev.type == "cuda", "MeldEngine needs the module on the GPU"
        ps = self.params = _ParamSlab(plist, dev)
        self.slab, self.grad, self.exp_avg, self.exp_avg_sq, self.step_count = ps.slab, ps.grad, ps.exp_avg, ps.exp_avg_sq, ps.step
        self._params, self._offs, self.total, self._p = ps.params, ps.offs, ps.total, ps.view
        offs = ps.offs
        self.lr, self.wd = lr, weight_decay
        self.class_w = torch.tensor(class_weights, device=dev, dtype=torch.float32) if class_weights is not None else None
        # the stack entry points' pointer arrays [L][ndir] (the slabs never move: built once)
        def arrays(slab):
            base, n = slab.data_ptr(), self.ndir * self.L
            return [(C.c_void_p * n)(*[base + 4 * offs[4 * i + j] for i in range(n)]) for j in range(4)]
        self._w, self._g = arrays(self.slab), arrays(self.grad)
        self.n_adds = max(1, self.L - 1)                      # one Philox offset per inter-layer dropout call
        self.loss = torch.zeros(1, device=dev)
        self.alpha = None

    def _check_SB(self, S, B):
        if B > self.max_dialogues or S > 128:
            raise ValueError("MeldEngine: at most %d dialogues%s of at most 128 utterances per step (the LSTM kernels' dialogue tile and "
                             "the general2 attention kernel's sequence limit); got S = %d, B = %d — split the batch, or run the "
                             "module path (MELDLSTMModel under autograd, which chunks by itself)"
                             % (self.max_dialogues, _MAX_DIALOGUES_HINT if self.max_dialogues < ops.MAX_DIALOGUES else "", S, B))

    def _prepare(self, S, B):
        fit = self._fit(S, B)
        if fit == "same":
            return
        if fit == "grow":
            cS, cB = self._alloc_S, self._alloc_B
            lib = _lib.load()
            cfg = _lib.LstmStackCfg(cS, cB, self.Dm, self.He, self.L, self.p_lstm, 1)
            n_saved, n_ws = ops.lstm_sizes(cfg, self.packed, self.ndir)
            T, D2, Cn = cS * cB, self.D2, self.n_classes
            z = lambda n: torch.empty(n, device=self.dev, dtype=torch.float32)
            self._f = dict(emotions=z(T * D2), xq=z(T * D2), att=z(T * D2), alpha=z(cB * cS * cS), tanh_s=z(cB * cS * cS),
                           du=z(cB * cS * cS), hidden=z(T * D2), logits=z(T * Cn), log_prob=z(T * Cn), dlogits=z(T * Cn),
                           d_res=z(T * D2), d_att=z(T * D2), d_xq=z(T * D2), d_mem=z(T * D2), d_tr=z(T * D2), d_em=z(T * D2),
                           saved=z(n_saved), ws=z(n_ws), lin_ws=z(int(lib.ganffn_linear_bwd_workspace_floats(T, D2, D2)) + 64))
            self.ws2 = torch.zeros(4, device=self.dev, dtype=torch.float32)
        self.cfg_train = _lib.LstmStackCfg(S, B, self.Dm, self.He, self.L, self.p_lstm, 1)
        self.cfg_eval = _lib.LstmStackCfg(S, B, self.Dm, self.He, self.L, self.p_lstm, 0)
        self.alpha = self._f["alpha"][:B * S * S].view(B, S, S)

    def step(self, batch, train=True):
        """batch: text (S,B,D_m) float32, umask (B,S) float, label (B,S) int64 (qmask / acoustic are not read:
        train_MELD.py:71 feeds the text features alone).  Returns (loss tensor, log_prob (S,B,C)); the attention weights of the
        step are `self.alpha` (B,S,S).  train=False: forward + loss only (model.eval()): no parameter, moment or step-count change."""
        text, umask, label = batch["text"], batch["umask"], batch["label"]
        S, B = text.shape[:2]
        if text.shape[2] != self.Dm or text.dtype != torch.float32 or not text.is_contiguous() or not text.is_cuda:
            raise ValueError("MeldEngine: text must be a contiguous float32 (S, B, %d) tensor on the GPU (data.to_meld_batch makes "
                             "it so); got %s %s" % (self.Dm, tuple(text.shape), text.dtype))
        self._prepare(S, B)
        if not self.params.in_place():
            raise RuntimeError("a MELDLSTMModel parameter was re-allocated after the engine was built (.to() / "
                               "flatten_parameters): build MeldEngine after the last .to()")
        P, st = ops._ptr, ops._stream()
        T, D2, Cn = S * B, self.D2, self.n_classes
        f = self._f
        self._base_add = base = self.rng.next_add(self.n_adds)        # SITE_LSTM + l draws offset base + l
        rng = self.rng.state
        cfg = self.cfg_train if train else self.cfg_eval
        w_ih, w_hh, b_ih, b_hh = self._w
        n_t = 4 * self.ndir * self.L
        w_t, b_t, w_s, b_s = (self._p(n_t + j) for j in range(4))
        # ---- forward: LSTM stack -> transform -> general2 attention -> hardswish head -> loss       (model.py:546-560)
        # packed: lengths on the device, no host read; alive until the backward is enqueued.  The entry points: ops.lstm_family
        lengths = umask.sum(1).to(torch.int32) if self.packed else None
        ops.lstm_stack_fwd_raw(cfg, text, w_ih, w_hh, b_ih, b_hh, f["emotions"], f["saved"], f["ws"], rng, base, lengths=lengths,
                               ndir=self.ndir)
        ops.linear_fwd_raw(f["emotions"], w_t, b_t, f["xq"], T, D2, D2)
        a_flags = ops.ATTN_CAUSAL if self.causal else None        # causal: step t attends to the emotions of steps j <= t
        ops.general2_attention_fwd_raw(f["xq"], f["emotions"], umask, f["att"], f["alpha"], f["tanh_s"], S, B, D2, a_flags)
        _lib.call("ganffn_meld_head_fwd", P(f["emotions"]), P(f["att"]), P(w_s), P(b_s), P(f["hidden"]), P(f["logits"]), T, D2, Cn, st)
        log_prob = f["log_prob"][:T * Cn].view(S, B, Cn)
        ops.logsoftmax_nll_raw(f["logits"], label, umask, self.class_w, log_prob, self.loss, f["dlogits"] if train else None,
                               self.ws2, S, B, Cn)                                             # train_MELD.py:72-74, model.py:62-81
        if not train:
            return self.loss, log_prob
        # ---- backward (the LSTM's weight gradients accumulate: the slab is zeroed first)
        _lib.call("ganffn_zero_floats", P(self.grad), C.c_int64(self.total), st)
        g_t, gb_t, g_s, gb_s = (self._p(n_t + j, True) for j in range(4))
        _lib.call("ganffn_meld_head_bwd", P(f["dlogits"]), P(f["emotions"]), P(f["att"]), P(f["hidden"]), P(w_s), P(f["d_res"]),
                  P(f["d_att"]), P(g_s), P(gb_s), T, D2, Cn, st)
        ops.general2_attention_bwd_raw(f["d_att"], f["xq"], f["emotions"], umask, f["alpha"], f["tanh_s"], f["du"], f["d_xq"], f["d_mem"],
                                       S, B, D2, a_flags)
        ops.linear_bwd_raw(f["d_xq"], f["emotions"], w_t, f["d_tr"], g_t, gb_t, T, D2, D2, f["lin_ws"])
        # d emotions = the residual + the attention's memory side + its query side through transform
        ops.add3_raw(f["d_res"], f["d_mem"], f["d_tr"], f["d_em"], T * D2)
        g_ih, g_hh, gb_ih, gb_hh = self._g
        ops.lstm_stack_bwd_raw(cfg, f["d_em"], text, f["emotions"], w_ih, w_hh, None, g_ih, g_hh, gb_ih, gb_hh, f["saved"], f["ws"], rng,
                               base, lengths=lengths, ndir=self.ndir)
        self.params.all_reduce(self.pg)
        self.params.adam(self.lr, self.wd, self.world)
        return self.loss, log_prob
