"""The call lists of tests/test_hip_workspace_bounds.py: every encoder, head, LSTM and DialogueRNN call on buffers of exactly the size the library
reports, each followed by GUARD floats of a fixed bit pattern inside the same tensor.  After every call `visit(label, buffers)`
is handed the full tensors (guards included) the call could have written: the test checks the guards, a comparison of two
libraries hashes them."""
import types

import torch

GUARD = 256
PATTERN = 0x7FA5C3E1                     # a NaN: nothing may read a buffer before writing it either
WIDTHS = [(100, 10, 2048), (64, 4, 128)]   # (E, H, F): rowchain + n100 + tn100 kernels | the generic path
SHAPES = [(3, 1), (5, 3)]                  # (S, B): T = 3 takes every round-to-4 | more than one dialogue
L = 2
SEED, ADD = 20261018, 5
# (kind, E, D1, D2): generator head | discriminator head, one kernel per direction | discriminator head, GEMM chain
HEADS = {"gen": (0, 100, 512, 100), "disc-fused": (1, 100, 64, 16), "disc-unfused": (1, 100, 64, 32)}
HEAD_T = 3


def guarded(n, fill=None):
    """n floats (fill, or the pattern) followed by GUARD floats of the pattern, as one tensor"""
    t = torch.full((n + GUARD,), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    if fill is not None:
        t[:n] = fill.reshape(-1).to(t.device) if torch.is_tensor(fill) else fill
    return t


def guard_intact(t):
    return bool((t[-GUARD:].view(torch.int32) == PATTERN).all())


def encoder_case(E, H, F, S, B, train, n_layers=L, lengths=None, causal=False):
    return types.SimpleNamespace(E=E, H=H, F=F, S=S, B=B, L=n_layers, train=train, lengths=lengths, causal=causal)


def run_encoder_case(c, visit):
    """forward unsaved | forward saved | backward [1,L) then [0,1) | backward [0,L) with and without grads | _bwd_parts where
    supported | _fwd_pair | (eval, no lengths, not causal) one stream step and one stream extend with m = 2"""
    from gan_ffn_amd import ops
    import encoder_range_cases as RC
    slab, x, pe, dout = RC.inputs(c)
    cfg = ops.enc_cfg(c.S, c.B, c.E, c.H, c.L, F=c.F, train=c.train)
    n_saved, n_ws = ops.enc_sizes(cfg)
    n_out = c.S * c.B * c.E
    slab_d, x_d, pe_d = slab.cuda(), x.cuda(), pe.cuda()
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    key_len = None if c.lengths is None else torch.tensor(c.lengths, dtype=torch.int32, device="cuda")
    mask = dict(key_len=key_len, causal=c.causal)

    out, ws = guarded(n_out), guarded(n_ws)
    ops.encoder_fwd_raw(cfg, x_d, pe_d, slab_d, out[:n_out], None, ws[:n_ws], rng, ADD, **mask)
    visit("fwd unsaved", {"out": out, "ws": ws})

    out, saved, ws = guarded(n_out), guarded(n_saved), guarded(n_ws)
    ops.encoder_fwd_raw(cfg, x_d, pe_d, slab_d, out[:n_out], saved[:n_saved], ws[:n_ws], rng, ADD, **mask)
    visit("fwd saved", {"out": out, "saved": saved, "ws": ws})

    def backward(label, ranges, grads=True):
        dx, g, ws = guarded(n_out, dout), guarded(slab.numel(), 0.5) if grads else None, guarded(n_ws)
        for lo, hi in ranges:
            ops.encoder_bwd_raw(cfg, lo, hi, dx[:n_out], slab_d, None if g is None else g[:slab.numel()], saved[:n_saved], ws[:n_ws],
                                rng, ADD, True, **mask)
            visit("%s [%d,%d)" % (label, lo, hi), {"dx": dx, "ws": ws, "saved": saved, **({} if g is None else {"grads": g})})

    backward("bwd", [(1, c.L), (0, 1)])
    backward("bwd", [(0, c.L)])
    backward("bwd no grads", [(0, c.L)], grads=False)

    if ops.encoder_bwd_parts_supported(cfg) and not c.causal:
        dx, g, ws = guarded(n_out, dout), guarded(slab.numel(), 0.5), guarded(n_ws)
        _, stride, n_parts, off = ops.encoder_bwd_parts_raw(cfg, dx[:n_out], slab_d, g[:slab.numel()], saved[:n_saved], ws[:n_ws], rng, ADD,
                                                            True, key_len=key_len)
        assert n_parts >= 1 and off >= 0 and stride >= 0 and off + n_parts * stride <= n_ws, (off, n_parts, stride, n_ws)
        visit("bwd_parts", {"dx": dx, "grads": g, "ws": ws, "saved": saved})

    if ops.encoder_fwd_pair_supported(cfg) and not c.causal:
        n_pair = ops.encoder_fwd_pair_workspace_floats(cfg)
        out, out2, saved2, ws = guarded(n_out), guarded(n_out), guarded(n_saved), guarded(n_pair)
        ops.encoder_fwd_pair_raw(cfg, x_d, pe_d, slab_d, out[:n_out], out2[:n_out], saved2[:n_saved], ws[:n_pair], rng, ADD, key_len=key_len)
        visit("fwd_pair", {"out_eval": out, "out_train": out2, "saved": saved2, "ws": ws})

    if not c.train and c.lengths is None and not c.causal and c.S >= 3:
        # the cache is S positions for each of B slots; every slot takes one row, then two more
        n_cache, n_step = ops.stream_sizes(cfg, c.B)
        n_ext = ops.stream_extend_sizes(cfg, 2 * c.B)
        cache, ws, wsx = guarded(n_cache), guarded(n_step), guarded(n_ext)
        slot = torch.arange(c.B, dtype=torch.int32, device="cuda")
        pos = torch.zeros(c.B, dtype=torch.int32, device="cuda")
        out = guarded(c.B * c.E)
        ops.encoder_stream_step_raw(cfg, c.B, slot, pos, x_d[0].contiguous(), pe_d, slab_d, cache[:n_cache], out[:c.B * c.E], ws[:n_step])
        visit("stream step", {"out": out, "cache": cache, "ws": ws})
        pos += 1
        out = guarded(2 * c.B * c.E)
        count = torch.full((c.B,), 2, dtype=torch.int32, device="cuda")
        ops.encoder_stream_extend_raw(cfg, c.B, 2, slot, count, pos, x_d[1:3].contiguous(), pe_d, slab_d, cache[:n_cache],
                                      out[:2 * c.B * c.E], wsx[:n_ext])
        visit("stream extend", {"out": out, "cache": cache, "ws": wsx})
    torch.cuda.synchronize()


LSTM_FAMILIES = ["", "batch", "packed"]      # ops.lstm_family: each one's entry points are called here whatever B is
LSTM_SHAPES = [(1, 1), (3, 1), (5, 3), (5, 33)]   # (S, B): the first step is the last | one dialogue | three | two dialogue tiles
LSTM_CALLS = [(f, s, b) for f in LSTM_FAMILIES for s, b in LSTM_SHAPES if f or b <= 32]      # (the plain family: at most 32 dialogues)
LSTM_WIDTHS = [(12, 8), (4, 8)]             # (In, H): wider than H, narrower (the partial slabs are sized for the larger)
LSTM_LAYERS = [1, 3]                         # no between-layer region | both parities of the alternating gradient buffer


def lstm_lengths(S, B):
    """packed lengths: (1, 5, 3) at (5, 3); ragged with dialogues of length 1 (the first among them) otherwise"""
    return (1, 5, 3) if (S, B) == (5, 3) else tuple(1 + (3 * b) % S for b in range(B))


def lstm_case(family, S, B, In, H, n_layers, train, p=0.5, lengths=None):
    if family == "packed" and lengths is None:
        lengths = lstm_lengths(S, B)
    return types.SimpleNamespace(family=family, S=S, B=B, In=In, H=H, L=n_layers, train=train, p=p, lengths=lengths)


def run_lstm_case(c, visit):
    """layer forward | layer backward (layer 0's weights) | stack forward | stack backward, through the entry points and the size
    functions of c.family"""
    import ctypes as C
    from gan_ffn_amd import _lib, ops
    lib, names = _lib.load(), ops._LSTM_ENTRY[c.family]
    gen = torch.Generator().manual_seed(SEED)
    rnd = lambda scale, *shape: ((torch.rand(*shape, generator=gen) - 0.5) * scale).cuda()
    S, B, In, H = c.S, c.B, c.In, c.H
    x, d_out = rnd(1.0, S, B, In), rnd(1.0, S, B, 2 * H)
    # [L][2] rows of w_ih, w_hh, b_ih, b_hh; the gradients start from 0.5 (they accumulate), each in a guarded tensor of its own
    W = [[rnd(0.6, 4 * H, In if l == 0 else 2 * H), rnd(0.6, 4 * H, H), rnd(0.2, 4 * H), rnd(0.2, 4 * H)] for l in range(c.L) for _ in range(2)]
    G = [[guarded(t.numel(), 0.5) for t in row] for row in W]
    arrays = lambda rows, n_rows: [ops._ptr_array([r[j] for r in rows[:n_rows]]) for j in range(4)]
    grads = lambda n_rows: [ops._ptr_array([g[j][:w[j].numel()] for g, w in zip(G[:n_rows], W)]) for j in range(4)]
    named = lambda n_rows: {"g%s[%d]" % (k, i): G[i][j] for i in range(n_rows) for j, k in enumerate(("w_ih", "w_hh", "b_ih", "b_hh"))}
    lengths = None if c.lengths is None else torch.tensor(c.lengths, dtype=torch.int32, device="cuda")
    P, st = ops._ptr, ops._stream()
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")

    def sizes(kind, cfg):
        n = tuple(int(getattr(lib, names[kind + "_sizes"] + w)(C.byref(cfg))) for w in ("saved_floats", "workspace_floats"))
        assert n[0] > 0 and n[1] > 0, (kind, n)
        return n

    def call(kind, what, cfg, *args):
        _lib.call(names[kind] + what, C.byref(cfg), *(() if lengths is None else (P(lengths),)), *args)

    n_out, n_dx = S * B * 2 * H, S * B * In
    for kind, cfg, n_rows, tail in (("layer", _lib.LstmCfg(S, B, In, H), 2, (st,)),
                                    ("stack", _lib.LstmStackCfg(S, B, In, H, c.L, c.p, int(c.train)), 2 * c.L, (P(rng), C.c_uint64(ADD), st))):
        n_saved, n_ws = sizes(kind, cfg)
        out, saved, ws = guarded(n_out), guarded(n_saved), guarded(n_ws)
        call(kind, "fwd", cfg, P(x), *arrays(W, n_rows), P(out[:n_out]), P(saved[:n_saved]), P(ws[:n_ws]), *tail)
        visit(kind + " fwd", {"out": out, "saved": saved, "ws": ws})
        dx, ws = guarded(n_dx), guarded(n_ws)
        call(kind, "bwd", cfg, P(d_out), P(x), P(out[:n_out]), *arrays(W, n_rows)[:2], P(dx[:n_dx]), *grads(n_rows), P(saved[:n_saved]),
             P(ws[:n_ws]), *tail)
        visit(kind + " bwd", {"dx": dx, "ws": ws, "saved": saved, "out": out, **named(n_rows)})
    torch.cuda.synchronize()


DRNN_WIDTHS = {"chain": (12, 8, 4), "per-step": (8, 8, 132)}      # (D_m, D_g = D_p, D_e): emotion chain | per-step cell, D_e > 2 D_g
DRNN_DA = 4
# (S, B, ndir, train, width, attention, listener, parties) — not the full product: every entry-point family (ops.drnn_family),
# every attention type with and without the listener, 1 / 2 / 16 parties, both width rows, every shape, both ndir, eval and train.
# dot needs D_m == D_g (the per-step row); general2 at S = 3, B = 1 has TS = 9 floats rounded to 12; 16 parties with the
# listener is the wide skinny group (34 problems in a launch), with 33 dialogues its tiled form.
DRNN_CASES = [
    (1, 1, 1, False, "chain", "general", False, 2), (3, 1, 2, True, "chain", "general", True, 2),
    (5, 3, 2, True, "chain", "general", False, 2), (5, 3, 1, False, "per-step", "general", False, 2),
    (5, 3, 2, True, "per-step", "general", True, 2), (1, 1, 2, False, "per-step", "general", False, 2),
    (3, 1, 1, False, "chain", "general2", False, 2), (3, 1, 2, True, "chain", "general2", True, 2),
    (5, 3, 1, True, "chain", "simple", False, 2), (5, 3, 2, False, "chain", "simple", True, 2),
    (5, 3, 1, False, "per-step", "dot", False, 2), (3, 1, 2, True, "per-step", "dot", True, 2),
    (5, 3, 2, True, "chain", "concat", False, 2), (5, 3, 1, False, "per-step", "concat", True, 2),
    (5, 3, 1, True, "chain", "general", False, 1), (5, 3, 2, False, "chain", "general", True, 1),
    (5, 3, 2, True, "per-step", "general", True, 16), (1, 1, 1, True, "per-step", "general2", False, 16),
    (5, 33, 2, True, "chain", "general", False, 2), (5, 33, 1, False, "per-step", "concat", True, 2),
    (5, 33, 2, True, "per-step", "general", True, 16)]
DRNN_LENGTHS = {(5, 3): (5, 3, 1)}            # a padded tail (mval 0, U 0) at (5, 3); full dialogues elsewhere


def drnn_case_id(case):
    S, B, ndir, train, width, att, listener, parties = case
    return "%dx%d-ndir%d-%s-%s-%s%s-P%d" % (S, B, ndir, "train" if train else "eval", width, att, "-listener" if listener else "", parties)


def run_drnn_case(case, visit, p=0.5):
    """forward | backward of ndir directions through ops.drnn_fwd_raw / drnn_bwd_raw (ops.drnn_family picks the entry points), every
    written buffer guarded: e, alpha, saved, ws and dU per direction, every gradient tensor on its own (started from 0.5).  The
    backward gets a fresh workspace: it may read alpha and saved, nothing the forward left in ws."""
    from gan_ffn_amd import _lib, ops
    S, B, ndir, train, width, att, listener, P = case
    Dm, H, He = DRNN_WIDTHS[width]
    Da = DRNN_DA if att == "concat" else 0
    gen = torch.Generator().manual_seed(SEED)
    rnd = lambda scale, *shape: ((torch.rand(*shape, generator=gen) - 0.5) * scale).cuda()
    lens = torch.tensor(DRNN_LENGTHS.get((S, B), (S,) * B))
    valid = (torch.arange(S).unsqueeze(1) < lens.unsqueeze(0)).float()               # (S, B)
    cell = lambda Hc, In: [rnd(0.6, 3 * Hc, In), rnd(0.6, 3 * Hc, Hc), rnd(0.2, 3 * Hc), rnd(0.2, 3 * Hc)]
    att_shapes = {"general": [(H, Dm)], "simple": [(1, H)], "dot": [], "general2": [(H, Dm), (H,)], "concat": [(Da, H + Dm), (1, Da)]}[att]
    U, spk, mval, prm, aprm, lprm = [], [], [], [], [], []
    for z in range(ndir):
        U.append((rnd(1.0, S, B, Dm) * valid.cuda().unsqueeze(2)).contiguous())
        spk.append(torch.randint(0, P, (S, B), generator=gen).to(torch.int32).cuda())
        mval.append(valid.cuda().contiguous())
        aprm.append([rnd(0.6, *s) for s in att_shapes])
        # the 13th cell tensor is general's transform.weight (the attention's own parameter); no other type has one
        prm.append(cell(H, Dm + H) + cell(H, Dm + H) + cell(He, H)[:1] + cell(He, He)[1:] + [aprm[z][0] if att == "general" else None])
        lprm.append(cell(H, Dm + H))
    if not listener:
        lprm = None
    cfg = _lib.DrnnCfg(S, B, Dm, H, He, p, int(train))
    acfg = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], Da)
    n_saved, n_ws = ops.drnn_floats(cfg, acfg, listener, P)
    n_e, n_al, n_u = S * B * He, B * S * S, S * B * Dm
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    A, att_ptrs = ops._ptr_array, lambda a, _: ops._att_ptrs(att, a)
    front = lambda ts, n: A([t[:n] for t in ts])
    structs = lambda cls, rows, fill=ops._drnn_ptrs: ops._ptr_structs(cls, rows, fill)
    PRM, LP, AP = structs(_lib.DrnnPtrs, prm), structs(_lib.DrnnListenerPtrs, lprm), structs(_lib.DrnnAttPtrs, aprm, att_ptrs)

    e, alpha = [guarded(n_e) for _ in range(ndir)], [guarded(n_al) for _ in range(ndir)]
    saved, ws = [guarded(n_saved) for _ in range(ndir)], [guarded(n_ws) for _ in range(ndir)]
    ops.drnn_fwd_raw(cfg, acfg, P, ndir, A(U), A(spk), A(mval), PRM, LP, AP, front(e, n_e), front(alpha, n_al), front(saved, n_saved),
                     front(ws, n_ws), ops._ptr(rng), ADD)
    named = lambda **k: {"%s[%d]" % (n, z): t for n, ts in k.items() for z, t in enumerate(ts)}
    visit("fwd", named(e=e, alpha=alpha, saved=saved, ws=ws))
    for z in range(ndir):
        assert bool(torch.isfinite(e[z][:n_e]).all()), "e[%d]" % z

    d_e = [rnd(1.0, S, B, He) for _ in range(ndir)]
    dU, ws = [guarded(n_u) for _ in range(ndir)], [guarded(n_ws) for _ in range(ndir)]
    guard_rows = lambda rows: [[None if t is None else guarded(t.numel(), 0.5) for t in r] for r in rows]
    G, AG, LG = guard_rows(prm), guard_rows(aprm), guard_rows(lprm) if listener else None
    for z in range(ndir):
        if att == "general":              # one tensor under both names, as its parameter
            AG[z][0] = G[z][12]
    fronts = lambda g_rows, rows: [[None if g is None else g[:t.numel()] for g, t in zip(gr, r)] for gr, r in zip(g_rows, rows)]
    ops.drnn_bwd_raw(cfg, acfg, P, ndir, A(d_e), A(U), A(spk), A(mval), PRM, LP, AP, structs(_lib.DrnnPtrs, fronts(G, prm)),
                     structs(_lib.DrnnListenerPtrs, fronts(LG, lprm)) if listener else None,
                     structs(_lib.DrnnAttPtrs, fronts(AG, aprm), att_ptrs), front(dU, n_u), front(alpha, n_al), front(saved, n_saved),
                     front(ws, n_ws), ops._ptr(rng), ADD)
    grads = {}
    for name, rows, of in (("g", G, prm), ("ag", AG, aprm)) + ((("lg", LG, lprm),) if listener else ()):
        grads.update({"%s[%d][%d]" % (name, z, j): (g, t.numel()) for z, (gr, r) in enumerate(zip(rows, of)) for j, (g, t) in enumerate(zip(gr, r))
                      if g is not None})
    visit("bwd", {**named(dU=dU, ws=ws, saved=saved, alpha=alpha), **{k: g for k, (g, _) in grads.items()}})
    for z in range(ndir):
        assert bool(torch.isfinite(dU[z][:n_u]).all()), "dU[%d]" % z
    for k, (g, n) in grads.items():
        assert bool(torch.isfinite(g[:n]).all()), k
    torch.cuda.synchronize()


def run_head_case(name, train, visit, T=HEAD_T):
    from gan_ffn_amd import ops
    from head_cases import head_inputs
    kind, E, D1, D2 = HEADS[name]
    tensors, d_out, g0 = head_inputs(kind, T, E, D1, D2)
    cfg = ops.head_cfg(T, E, D1, D2, kind, 0.2, train)
    n_saved, n_ws = ops.head_sizes(cfg)
    n_out = T * (D2 if kind == 0 else 1)
    dt = [None if t is None else t.cuda() for t in tensors]
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    out, saved, ws = guarded(n_out), guarded(n_saved), guarded(n_ws)
    ops.head_fwd_raw(cfg, *dt, out[:n_out], saved[:n_saved], ws[:n_ws], rng, ADD)
    visit("head fwd", {"out": out, "saved": saved, "ws": ws})
    G = {k: guarded(v.numel(), v) for k, v in g0.items()}
    g = lambda k: G[k][:g0[k].numel()] if k in G else None
    dx = guarded(T * E)
    ops.head_bwd_raw(cfg, d_out.cuda(), dt[0], dt[1], dt[3], dt[5], g("w1"), g("b1"), g("w2"), g("b2"), g("w3"), g("b3"), dx[:T * E],
                     saved[:n_saved], ws[:n_ws], rng, ADD)
    visit("head bwd", {"dx": dx, "saved": saved, "ws": ws, **{"g" + k: v for k, v in G.items()}})
    torch.cuda.synchronize()
