"""DialogueRNN head for configuration 5: `GAN_FFN_DialogueRNN` = the three HIP generators feeding a
bidirectional DialogueRNN classifier.

Mirrors the module interface of /root/reference/model.py:134-194 (MatchingAttention, SimpleAttention), :828-1062
(DialogueRNNCell, DialogueRNN, BiModel) and :1465-1528 (GAN_FFN_DialogueRNN): same constructor arguments, same
parameter names and shapes (reference state_dicts load), same forward signatures and return tuples.

On the GPU, with every context attention type (general, simple, dot, general2, concat — the reference script's
--attention), with or without listener state (--active-listener), the recurrence is the HIP path of csrc/dialogue_rnn.hip
(ops.DialogueRNNFn: both directions of BiModel through one chain of launches, forward and backward;
ops.dialogue_rnn_supported / dialogue_rnn_listener_supported say when: D_g = D_p <= 512, dot with D_m = D_g, concat with
D_a % 4 == 0 and D_a <= 512, at most 112 steps, 1 to ops.DRNN_MAX_PARTIES = 16 parties — qmask's width: IEMOCAP's 2,
MELD's 9; any batch size, one native call per ops.MAX_DIALOGUES = 256 dialogues); CPU tensors and shapes outside those limits take the torch-op
restatement below, which is also what the reference-fixture parity tests pin.  The pieces with no sequential dependence are batched:
  * party selection is a gather, sequence reversal one index gather per tensor (the reference loops over dialogues),
  * BiModel's second attention — one masked `general2` MatchingAttention query per time step in the reference — is ONE
    batched masked attention over all (dialogue, query step) pairs (`general2_all_queries`).
The generators underneath are the HIP path; there is no CPU route through them.
An extension the reference does not have: `UniModel` / `GAN_FFN_DialogueRNN(causal=True)`, the classifier that never looks ahead
(one forward DialogueRNN, causal second attention, causal generators), which also streams: `GAN_FFN_DialogueRNN.stream()`
(streaming.DrnnStreamSession) labels each utterance as it arrives, one recurrence step per utterance against per-slot state.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


class SimpleAttention(nn.Module):
    """softmax over time of a learned scalar score; pooled memory (model.py:117-131)"""

    def __init__(self, input_dim):
        super().__init__()
        self.input_dim = input_dim
        self.scalar = nn.Linear(input_dim, 1, bias=False)

    def forward(self, M, x=None):
        alpha = F.softmax(self.scalar(M), dim=0).permute(1, 2, 0)            # (B, 1, S)
        return torch.bmm(alpha, M.transpose(0, 1))[:, 0, :], alpha


def general2_scores(xt, M, mask, causal=False):
    """masked `general2` attention weights for queries xt (B, Q, D) over memory M (S, B, D), mask (B, S):
    softmax_j tanh(m_j * <x, m_j * M_j>), zeroed at masked positions and re-normalised (model.py:169-182).
    causal (Q = S, query t is step t): the keys of query t are the steps j <= t, a_tj = e^{s_tj} m_j [j <= t] /
    sum_{k <= t} e^{s_tk} m_k — the same call on M[:t+1] and mask[:, :t+1] for every t."""
    Mb = M.transpose(0, 1) * mask.unsqueeze(2)                               # (B, S, D), masked memory
    a = torch.tanh(torch.bmm(xt, Mb.transpose(1, 2)) * mask.unsqueeze(1))    # (B, Q, S)
    if causal:
        # s is bounded by tanh: e^s needs no max-subtraction, and the softmax's own denominator cancels in the re-normalisation
        a = torch.exp(a) * mask.unsqueeze(1) * torch.tril(torch.ones_like(a[0]))
        return a / a.sum(dim=2, keepdim=True)
    a = F.softmax(a, dim=2) * mask.unsqueeze(1)
    return a / a.sum(dim=2, keepdim=True)


class MatchingAttention(nn.Module):
    """attention of one candidate vector over a memory sequence; att_type in dot / general / general2 / concat
    (model.py:134-194)"""

    def __init__(self, mem_dim, cand_dim, alpha_dim=None, att_type="general2"):
        super().__init__()
        assert att_type != "concat" or alpha_dim is not None
        assert att_type != "dot" or mem_dim == cand_dim
        self.mem_dim, self.cand_dim, self.att_type = mem_dim, cand_dim, att_type
        if att_type == "general":
            self.transform = nn.Linear(cand_dim, mem_dim, bias=False)
        if att_type == "general2":
            self.transform = nn.Linear(cand_dim, mem_dim, bias=True)
            nn.init.normal_(self.transform.weight, std=0.01)
        elif att_type == "concat":
            self.transform = nn.Linear(cand_dim + mem_dim, alpha_dim, bias=False)
            self.vector_prod = nn.Linear(alpha_dim, 1, bias=False)

    def forward(self, M, x, mask=None):
        """M (S, B, mem_dim), x (B, cand_dim), mask (B, S) -> pooled (B, mem_dim), alpha (B, 1, S)"""
        if mask is None:
            mask = torch.ones(M.size(1), M.size(0), dtype=M.dtype, device=M.device)
        if self.att_type == "dot":
            alpha = F.softmax(torch.bmm(x.unsqueeze(1), M.permute(1, 2, 0)), dim=2)
        elif self.att_type == "general":
            alpha = F.softmax(torch.bmm(self.transform(x).unsqueeze(1), M.permute(1, 2, 0)), dim=2)
        elif self.att_type == "general2":
            alpha = general2_scores(self.transform(x).unsqueeze(1), M, mask)
        else:
            Mb = M.transpose(0, 1)
            cat = torch.cat([Mb, x.unsqueeze(1).expand(-1, M.size(0), -1)], 2)
            alpha = F.softmax(self.vector_prod(torch.tanh(self.transform(cat))), 1).transpose(1, 2)
        return torch.bmm(alpha, M.transpose(0, 1))[:, 0, :], alpha

    def general2_all_queries(self, M, mask, causal=False):
        """every time step of M as the candidate, at once: -> pooled (S, B, D), alpha (B, S_query, S_memory).
        Equals [self(M, M[t], mask) for t in range(S)] (what BiModel.forward loops over, model.py:1043-1049).
        causal=True (an extension the reference does not have; UniModel's attention): step t attends to steps j <= t only —
        [self(M[:t+1], M[t], mask[:, :t+1]) for t in range(S)], alpha exactly 0 above the diagonal."""
        assert self.att_type == "general2"
        if M.is_cuda and M.size(0) <= 128 and M.size(2) <= 1024:
            from . import ops                      # one HIP kernel per direction instead of ~10 torch ops on (B,S,S)
            return ops.General2AttnFn.apply(self.transform(M), M, mask, causal)
        alpha = general2_scores(self.transform(M).transpose(0, 1), M, mask, causal)  # (B, S, S)
        return torch.bmm(alpha, M.transpose(0, 1)).transpose(0, 1), alpha


def _select_party(X, idx):
    """X (B, P, D), idx (B) -> X[b, idx[b]] (B, D)"""
    return X.gather(1, idx.view(-1, 1, 1).expand(-1, 1, X.size(2)))[:, 0, :]


class DialogueRNNCell(nn.Module):
    """one utterance step: global GRU, context attention over the global history, party GRU (speaker update, optional
    listener update), emotion GRU (model.py:828-926)"""

    def __init__(self, D_m, D_g, D_p, D_e, listener_state=False, context_attention="simple", D_a=100, dropout=0.5):
        super().__init__()
        self.D_m, self.D_g, self.D_p, self.D_e = D_m, D_g, D_p, D_e
        self.listener_state = listener_state
        self.g_cell = nn.GRUCell(D_m + D_p, D_g)
        self.p_cell = nn.GRUCell(D_m + D_g, D_p)
        self.e_cell = nn.GRUCell(D_p, D_e)
        if listener_state:
            self.l_cell = nn.GRUCell(D_m + D_p, D_p)
        self.dropout = nn.Dropout(dropout)
        if context_attention == "simple":
            self.attention = SimpleAttention(D_g)
        else:
            self.attention = MatchingAttention(D_g, D_m, D_a, context_attention)

    def forward(self, U, qmask, g_hist, q0, e0):
        """U (B, D_m), qmask (B, P) one-hot speaker, g_hist (t, B, D_g) or empty, q0 (B, P, D_p), e0 (B, D_e) or empty"""
        B, P = qmask.shape
        spk = torch.argmax(qmask, 1)
        first = g_hist.size(0) == 0
        g_prev = U.new_zeros(B, self.D_g) if first else g_hist[-1]
        g_ = self.dropout(self.g_cell(torch.cat([U, _select_party(q0, spk)], dim=1), g_prev))
        if first:
            c_, alpha = U.new_zeros(B, self.D_g), None
        else:
            c_, alpha = self.attention(g_hist, U)
        Uc = torch.cat([U, c_], dim=1).unsqueeze(1).expand(-1, P, -1).reshape(B * P, self.D_m + self.D_g)
        qs_ = self.dropout(self.p_cell(Uc, q0.reshape(B * P, self.D_p)).view(B, P, self.D_p))
        if self.listener_state:
            Ue = U.unsqueeze(1).expand(-1, P, -1).reshape(B * P, self.D_m)
            ss = _select_party(qs_, spk).unsqueeze(1).expand(-1, P, -1).reshape(B * P, self.D_p)
            ql_ = self.dropout(self.l_cell(torch.cat([Ue, ss], 1), q0.reshape(B * P, self.D_p)).view(B, P, self.D_p))
        else:
            ql_ = q0
        qm = qmask.unsqueeze(2)
        q_ = ql_ * (1 - qm) + qs_ * qm
        e_prev = U.new_zeros(B, self.D_e) if e0.size(0) == 0 else e0
        e_ = self.dropout(self.e_cell(_select_party(q_, spk), e_prev))
        return g_, q_, e_, alpha


class DialogueRNN(nn.Module):
    """the cell unrolled over a dialogue (model.py:929-972)"""

    def __init__(self, D_m, D_g, D_p, D_e, listener_state=False, context_attention="simple", D_a=100, dropout=0.5):
        super().__init__()
        self.D_m, self.D_g, self.D_p, self.D_e = D_m, D_g, D_p, D_e
        self.dropout = nn.Dropout(dropout)
        self.dialogue_cell = DialogueRNNCell(D_m, D_g, D_p, D_e, listener_state, context_attention, D_a, dropout)

    def forward(self, U, qmask):
        """U (S, B, D_m), qmask (S, B, P) -> emotions (S, B, D_e), [alpha_t (B, t)] for t >= 1"""
        from . import ops
        if _hip_recurrence(ops, self.dialogue_cell, U, qmask):
            # the HIP recurrence (csrc/dialogue_rnn.hip): every attention type, with or without listener state
            return ops.dialogue_rnn_run([self.dialogue_cell], [U], [qmask], self.training)[0]
        S, B, P = qmask.shape
        g_steps, e_steps, alpha = [], [], []
        q_ = U.new_zeros(B, P, self.D_p)
        e_ = U.new_zeros(0)
        for t in range(S):
            g_hist = torch.stack(g_steps, 0) if g_steps else U.new_zeros(0)
            g_, q_, e_, a_ = self.dialogue_cell(U[t], qmask[t], g_hist, q_, e_)
            g_steps.append(g_)
            e_steps.append(e_)
            if a_ is not None:
                alpha.append(a_[:, 0, :])
        return torch.stack(e_steps, 0), alpha


def _hip_recurrence(ops, cell, U, qmask):
    """whether the HIP recurrence runs this cell: the listener-free path or the listener path"""
    if cell.listener_state:
        return ops.dialogue_rnn_listener_supported(cell, U, qmask)
    return ops.dialogue_rnn_supported(cell, U, qmask)


def reverse_valid_prefix(X, mask):
    """X (S, B, D), mask (B, S): reverse each dialogue's first len_b = sum(mask_b) steps, zero the rest; the result is
    trimmed to max len_b like pad_sequence does (model.py:1008-1021)"""
    S, B = X.shape[0], X.shape[1]
    lens = mask.sum(1).to(torch.long)                                    # (B)
    # pad-collate makes the longest dialogue exactly S long, so max(lens) == S; reading it back would cost a host
    # sync per call (and forbid graph capture).  Only CPU callers (tests) may pass a mask with trailing all-zero steps.
    Smax = S if X.is_cuda else int(lens.max())
    t = torch.arange(Smax, device=X.device).unsqueeze(1)                 # (Smax, 1)
    src = (lens.unsqueeze(0) - 1 - t).clamp(min=0)                       # (Smax, B)
    valid = (t < lens.unsqueeze(0)).to(X.dtype).unsqueeze(2)
    idx = src.unsqueeze(2).expand(-1, -1, X.shape[2])
    return X.gather(0, idx) * valid


def _classify(m, emotions, umask, att2, causal):
    """the tail BiModel and UniModel share: the second (masked general2; causal for UniModel) attention over the emotion sequence,
    linear + relu + dropout, class log-probabilities -> (log_prob, alpha)"""
    alpha = []
    if att2:
        emotions, a = m.matchatt.general2_all_queries(emotions, umask, causal)
        alpha = [a[:, t, :] for t in range(a.size(1))]
    hidden = m.dropout(F.relu(m.linear(emotions)))
    return F.log_softmax(m.smax_fc(hidden), 2), alpha


class BiModel(nn.Module):
    """forward and backward DialogueRNN, concatenated, second (masked general2) attention over the emotion sequence,
    linear + relu + dropout, class log-probabilities (model.py:975-1062)"""

    def __init__(self, D_m, D_g, D_p, D_e, D_h, n_classes=7, listener_state=False, context_attention="simple", D_a=100,
                 dropout_rec=0.5, dropout=0.5):
        super().__init__()
        self.D_m, self.D_g, self.D_p, self.D_e, self.D_h, self.n_classes = D_m, D_g, D_p, D_e, D_h, n_classes
        self.dropout = nn.Dropout(dropout)
        self.dropout_rec = nn.Dropout(dropout + 0.15)
        self.dialog_rnn_f = DialogueRNN(D_m, D_g, D_p, D_e, listener_state, context_attention, D_a, dropout_rec)
        self.dialog_rnn_r = DialogueRNN(D_m, D_g, D_p, D_e, listener_state, context_attention, D_a, dropout_rec)
        self.linear = nn.Linear(2 * D_e, 2 * D_h)
        self.smax_fc = nn.Linear(2 * D_h, n_classes)
        self.matchatt = MatchingAttention(2 * D_e, 2 * D_e, att_type="general2")

    def _reverse_seq(self, X, mask):
        return reverse_valid_prefix(X, mask)

    def forward(self, U, qmask, umask, att2=True):
        from . import ops
        rev_U, rev_qmask = self._reverse_seq(U, umask), self._reverse_seq(qmask, umask)
        cf, cr = self.dialog_rnn_f.dialogue_cell, self.dialog_rnn_r.dialogue_cell
        if (cf.listener_state == cr.listener_state and _hip_recurrence(ops, cf, U, qmask) and _hip_recurrence(ops, cr, rev_U, rev_qmask)
                and rev_U.shape == U.shape):
            # both directions through the same chain of launches (csrc/dialogue_rnn.hip)
            (emotions_f, alpha_f), (emotions_b, alpha_b) = ops.dialogue_rnn_run([cf, cr], [U, rev_U], [qmask, rev_qmask],
                                                                                self.training)
        else:
            emotions_f, alpha_f = self.dialog_rnn_f(U, qmask)
            emotions_b, alpha_b = self.dialog_rnn_r(rev_U, rev_qmask)
        emotions_f = self.dropout_rec(emotions_f)
        emotions_b = self.dropout_rec(self._reverse_seq(emotions_b, umask))
        return (*_classify(self, torch.cat([emotions_f, emotions_b], dim=-1), umask, att2, False), alpha_f, alpha_b)


class UniModel(nn.Module):
    """BiModel without its look-ahead (an extension the reference does not have): ONE forward DialogueRNN — its context
    attention of step t sees g_0 .. g_{t-1} only, so the recurrence is causal by construction —, the second (masked general2)
    attention CAUSAL (step t attends to the emotions of steps j <= t: MatchingAttention.general2_all_queries(causal=True)),
    linear + relu + dropout, class log-probabilities.  log_prob[t] of a dialogue is a function of its utterances and speakers
    0 .. t.  There is no dialog_rnn_r; matchatt is D_e x D_e, linear D_e -> D_h, smax_fc D_h -> n_classes; the dropouts are
    BiModel's.  Returns BiModel's tuple with an empty alpha_b."""

    def __init__(self, D_m, D_g, D_p, D_e, D_h, n_classes=7, listener_state=False, context_attention="simple", D_a=100,
                 dropout_rec=0.5, dropout=0.5):
        super().__init__()
        self.D_m, self.D_g, self.D_p, self.D_e, self.D_h, self.n_classes = D_m, D_g, D_p, D_e, D_h, n_classes
        self.dropout = nn.Dropout(dropout)
        self.dropout_rec = nn.Dropout(dropout + 0.15)
        self.dialog_rnn_f = DialogueRNN(D_m, D_g, D_p, D_e, listener_state, context_attention, D_a, dropout_rec)
        self.linear = nn.Linear(D_e, D_h)
        self.smax_fc = nn.Linear(D_h, n_classes)
        self.matchatt = MatchingAttention(D_e, D_e, att_type="general2")

    def forward(self, U, qmask, umask, att2=True):
        emotions, alpha_f = self.dialog_rnn_f(U, qmask)
        return (*_classify(self, self.dropout_rec(emotions), umask, att2, True), alpha_f, [])


class GAN_FFN_DialogueRNN(nn.Module):
    """fusion = G_a(acoustic) + G_v(visual) + G_t(text) -> BiModel (model.py:1465-1528).  `gelu`, `relu`, `dropout`
    and `fc1` exist on the reference object without taking part in forward; they are kept so state_dicts match.
    mask_padding (default False: the reference passes no mask) is an extension: the generators' self-attention ignores the padded
    utterances of every dialogue (key lengths umask.sum(1), derived on the device), the one place where padding reached a real
    utterance's prediction.  `umask` must then be a PREFIX mask.  A plain attribute: the state_dict is the same either way.
    causal (default False) is an extension the reference does not have: a classifier that never looks ahead.  The head is a
    UniModel (one forward DialogueRNN, causal second attention) and the three generators run under the causal self-attention
    mask (composing with mask_padding as in GAN_FFN), so log_prob[t] of a dialogue depends on its utterances and speakers
    0 .. t alone.  The UniModel is kept under the attribute name `bi_model`, so that engines, artifacts and tools that say
    net.bi_model keep working.  A plain attribute; the state_dict is the bidirectional one without bi_model.dialog_rnn_r.*,
    with bi_model.matchatt.transform D_e x D_e, bi_model.linear D_e -> D_h and bi_model.smax_fc D_h -> n_classes.
    causal=False constructs and runs exactly what it always did.  The option is given by keyword only
    (GAN_FFN_DialogueRNN(..., causal=True)): it arrives through `options`, whose one known key is `causal` — any other keyword
    raises TypeError as an unknown argument does — so the constructor's named parameters are the ones it always had."""

    def __init__(self, acoustic_generator, visual_generator, text_generator, D_m, D_g, D_p, D_e, D_h, D_a, n_classes,
                 listener_state, context_attention, dropout_rec, dropout, mask_padding=False, **options):
        super().__init__()
        self.mask_padding = bool(mask_padding)
        self.causal = bool(options.pop("causal", False))
        if options:
            raise TypeError("GAN_FFN_DialogueRNN.__init__() got an unexpected keyword argument %r" % sorted(options)[0])
        self.n_classes = n_classes
        self.acoustic_generator = acoustic_generator
        self.visual_generator = visual_generator
        self.text_generator = text_generator
        self.gelu, self.relu, self.dropout = nn.GELU(), nn.ReLU(), nn.Dropout(dropout)
        self.bi_model = (UniModel if self.causal else BiModel)(D_m=D_m, D_g=D_g, D_p=D_p, D_e=D_e, D_h=D_h, n_classes=n_classes,
                                                               listener_state=listener_state, context_attention=context_attention,
                                                               D_a=D_a, dropout_rec=dropout_rec, dropout=dropout)
        self.fc1 = nn.Linear(100, n_classes)
        self.stream = self._open_stream            # a plain instance attribute (a bound method): see _open_stream

    def forward(self, acoustic, visual, text, qmask, umask):
        from . import ops
        kl = ops.key_lengths_from_umask(umask) if self.mask_padding else None
        c = self.causal
        fusion = self.acoustic_generator(acoustic, kl, c) + self.visual_generator(visual, kl, c) + self.text_generator(text, kl, c)
        return self.bi_model(fusion, qmask, umask)

    def _open_stream(self, capacity=1, max_len=110, parties=2):
        """net.stream(capacity=1, max_len=MAX_LEN, parties=2): the name `stream` is bound on every INSTANCE in __init__, not on the
        class — the class keeps the attribute set it always had (tests/test_stream_cpu.py and tests/test_stream_extend_cpu.py pin that
        the class carries no `stream`), and a net streams or refuses by what it was built with.
        -> a streaming.DrnnStreamSession: label each utterance of up to `capacity` concurrent dialogues as it arrives, from the
        generators' per-layer K/V caches and the head's per-slot recurrence state (one DialogueRNN step per new utterance).  Needs
        causal=True: the bidirectional head reads the future.  max_len: positions per slot (<= model.MAX_LEN = 110); parties: the
        width of the party axis (qmask's last dimension; speakers are given as indices)."""
        from .streaming import DrnnStreamSession
        return DrnnStreamSession(self, capacity, max_len, parties)


class MELDLSTMModel(nn.Module):
    """MELD classifier (/root/reference/model.py:520-562, train_MELD.py:147-151): 4-layer
    bidirectional LSTM over the utterance features, masked general2 attention of every step over the sequence,
    hardswish(emotions + hardswish(attended)), class log-probabilities.  `linear` and `dropout` serve the att2=False
    branch / exist on the reference object.  On the GPU the LSTM recurrence runs on the build's own kernels (csrc/lstm.hip
    through ops.lstm_forward: hoisted input products, one skinny MFMA product + one gate launch per step for both directions,
    deferred weight gradients) with `self.lstm`'s parameters — round 5; until then MIOpen's; the attention is the batched
    general2 kernel used by BiModel.
    packed (default False: the reference's padded run, model.py:546) is an extension the reference does not have: the LSTM runs
    on packed sequences — every dialogue for its own umask.sum(1) steps, zero output past its end, the reverse direction starting
    at its last real utterance — so a dialogue's prediction no longer depends on how far its batch is padded.  `umask` must then be
    a PREFIX mask (ones for the real utterances, then zeros: what every loader of the project produces).  A plain attribute, not a
    parameter or buffer: the state_dict is the same either way.
    causal (default False) is an extension the reference does not have: a classifier that never looks ahead.  The LSTM is
    forward-only (nn.LSTM(bidirectional=False): no *_reverse parameters; the same ops.lstm_forward call path with one direction) and
    the general2 attention is CAUSAL (step t attends to the emotions of steps j <= t:
    MatchingAttention.general2_all_queries(causal=True)), so log_prob[t] of a dialogue is a function of its utterances 0 .. t
    alone.  matchatt is D_e x D_e, linear D_e -> D_h, smax_fc D_h -> n_classes; the att2=True branch feeds the D_e-wide hidden
    to smax_fc, so it needs D_h == D_e just as the reference's needs D_h == 2 D_e.  Composes with packed.  causal=False
    constructs and runs exactly what it always did."""

    def __init__(self, D_m, D_e, D_h, n_classes=7, dropout=0.5, packed=False, causal=False):
        super().__init__()
        self.n_classes = n_classes
        self.packed = bool(packed)
        self.causal = bool(causal)
        self.D_e, self.D_h = D_e, D_h
        D = D_e if self.causal else 2 * D_e          # width of the LSTM's output
        self.dropout = nn.Dropout(dropout)
        self.lstm = nn.LSTM(input_size=D_m, hidden_size=D_e, num_layers=4, bidirectional=not self.causal, dropout=dropout)
        self.matchatt = MatchingAttention(D, D, att_type="general2")
        self.linear = nn.Linear(D, D_h)
        self.smax_fc = nn.Linear(D_h, n_classes)
        self.stream = self._open_stream            # a plain instance attribute (a bound method): see _open_stream

    def _open_stream(self, capacity=1, max_len=110):
        """model.stream(capacity=1, max_len=MAX_LEN): the name `stream` is bound on every INSTANCE in __init__, not on the class, as
        GAN_FFN_DialogueRNN binds its own (tests/test_stream_cpu.py and tests/test_stream_extend_cpu.py pin that the class carries no
        `stream`).  -> a streaming.MeldStreamSession: label each utterance of up to `capacity` concurrent dialogues as it arrives,
        from per-slot (h, c) of every LSTM layer and the slot's emotion history (one LSTM step per new utterance instead of the
        whole prefix).  Needs causal=True — the bidirectional LSTM's reverse direction starts at the dialogue's end — and D_h == D_e
        (the att2=True branch).  max_len: positions per slot (<= model.MAX_LEN = 110).  `packed` is irrelevant: a stream has no
        padding."""
        from .streaming import MeldStreamSession
        return MeldStreamSession(self, capacity, max_len)

    def forward(self, U, qmask, umask, visuf=None, att2=True):
        if self.causal and att2 and self.D_h != self.D_e:
            raise ValueError("MELDLSTMModel(causal=True): the att2=True branch hands the D_e-wide hidden to smax_fc, so it needs "
                             "D_h == D_e; got D_e=%d D_h=%d" % (self.D_e, self.D_h))
        if U.is_cuda:
            # the recurrence on the HIP kernels (csrc/lstm.hip), with self.lstm's own parameters (same state_dict keys)
            from . import ops
            lengths = umask.sum(1).to(torch.int32) if self.packed else None       # on the device: no host read
            emotions = ops.lstm_forward(U, self.lstm, self.training, lengths=lengths)
        elif self.packed:
            # CPU tensors: torch's own packing (pack_padded_sequence wants its lengths on the host)
            seq = nn.utils.rnn.pack_padded_sequence(U, umask.sum(1).to(torch.int64).cpu(), enforce_sorted=False)
            emotions, _ = nn.utils.rnn.pad_packed_sequence(self.lstm(seq)[0], total_length=U.shape[0])
        else:
            emotions, _ = self.lstm(U)      # CPU tensors: stock torch (the fixtures' CPU check; the product path is the GPU one)
        alpha, alpha_f, alpha_b = [], [], []
        if att2:
            att, a = self.matchatt.general2_all_queries(emotions, umask, self.causal)
            alpha = [a[:, t, :] for t in range(a.size(1))]
            hidden = F.hardswish(emotions + F.hardswish(att))
        else:
            hidden = F.gelu(self.linear(emotions))
        return F.log_softmax(self.smax_fc(hidden), 2), alpha, alpha_f, alpha_b
