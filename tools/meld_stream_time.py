"""Time the streaming causal MELD classifier (MELDLSTMModel(causal=True).stream) against the full-prefix forward and print one
JSON line.

Labels 33-utterance dialogues (MELD's longest) utterance by utterance at B = 1, 8 and 32 concurrent dialogues, all in one process,
the same model (trained widths 600 / 300 / 300) and inputs for every variant:
  (a) prefix : what a tree without the stream offers — model.eval() under no_grad on the prefix 0 .. t for every t;
  (b) stream : sess.step.
One block = one whole pass over the 33 utterances between two device synchronisations; two warm-up rounds, then `--repeats`
rounds in which the variants alternate block by block.  The JSON carries every block, the median and [min, max] of the totals (ms
per 33 utterances), the same for single calls at t = 0, 16, 32 (a device synchronisation before and after the call), and the
condition "the total of (b) at B = 32 is lower than (a) by more than the larger of the two min-max spreads".

--extend: reaching utterance 33 of a dialogue that is already under way, same protocol:
  (a) steps  : sess.reset(), then 33 x sess.step;
  (b) extend : sess.reset(), then sess.extend over the first 32 utterances and sess.step on the 33rd.
One block = reset to the label of utterance 33 between two device synchronisations; the condition is the same, at B = 32.

--kernels: the LSTM step alone (ganffn_stream_lstm_step: its 9 launches) and the native extend alone (ganffn_stream_lstm_extend
with m = 32: 32 x 9 launches) from position 32 / 0 with 32 rows, trained widths; device events around `--launches` calls captured
into one graph, microseconds per call.  Run it under a kernel trace for the per-kernel durations of the step's launches.

    python tools/meld_stream_time.py [--repeats 5] [--root DIR]
    python tools/meld_stream_time.py --extend [--repeats 5]
    python tools/meld_stream_time.py --kernels [--launches 200] [--repeats 5]

--root DIR imports the package from another checkout (with its own built library), e.g. the parent commit's: a tree without
`MELDLSTMModel.stream` is timed on (a) alone.
"""
import argparse
import json
import os
import statistics
import sys
import time

S = 33
PROBE_T = (0, 16, 32)
WARMUP_ROUNDS = 2
DIMS = (600, 300, 300)       # D_m, D_e, D_h: the trained widths


def summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "spread": round(max(v) - min(v), nd)}


def build_model(torch):
    from gan_ffn_amd import dialogue_rnn as DR
    torch.manual_seed(3407)
    return DR.MELDLSTMModel(*DIMS, n_classes=7, dropout=0.5, causal=True).cuda().eval()


def inputs(torch, B):
    g = torch.Generator().manual_seed(B)
    return (torch.rand(S, B, DIMS[0], generator=g) - 0.5).cuda(), torch.ones(B, S).cuda()


def sessions(args, torch):
    model = build_model(torch)
    has = hasattr(model, "stream")
    out = {"root": os.path.abspath(args.root), "S": S, "repeats": args.repeats, "has_stream": has, "totals_ms": {}, "blocks": {},
           "warmup_blocks": {}, "per_t_ms": {}}
    for B in (1, 8, 32):
        text, umask = inputs(torch, B)

        def prefix_call(u):
            return model(text[:u + 1], None, umask[:, :u + 1])[0]

        variants = {"prefix": prefix_call}
        sess = {}
        if has:
            sess["stream"] = model.stream(capacity=B)
            variants["stream"] = (lambda u, s=sess["stream"]: s.step(text[u]))

        def whole(name):
            if name in sess:
                sess[name].reset()
            fn = variants[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for u in range(S):
                fn(u)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def probed(name, acc):
            if name in sess:
                sess[name].reset()
            fn = variants[name]
            for u in range(S):
                if u in PROBE_T:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(u)
                    torch.cuda.synchronize()
                    acc.setdefault(u, []).append((time.perf_counter() - t0) * 1e3)
                else:
                    fn(u)

        with torch.no_grad():
            runs = {k: [] for k in variants}
            for r in range(args.repeats + WARMUP_ROUNDS):
                for k in variants:
                    runs[k].append(whole(k))
            per_t = {k: {} for k in variants}
            for r in range(args.repeats):
                for k in variants:
                    probed(k, per_t[k])
        for k, vals in runs.items():
            key = "B%d_%s" % (B, k)
            out["blocks"][key] = [round(x, 3) for x in vals[WARMUP_ROUNDS:]]
            out["warmup_blocks"][key] = [round(x, 3) for x in vals[:WARMUP_ROUNDS]]
            out["totals_ms"][key] = summary(vals[WARMUP_ROUNDS:])
            out["per_t_ms"][key] = {str(u): summary(x, 4) for u, x in per_t[k].items()}
        del sess
    if has:
        tm = out["totals_ms"]
        a_, b_ = tm["B32_prefix"], tm["B32_stream"]
        margin = max(a_["spread"], b_["spread"])
        out["condition_B32"] = {"prefix_median_ms": a_["median"], "stream_median_ms": b_["median"], "larger_spread_ms": margin,
                                "holds": bool(a_["median"] - b_["median"] > margin)}
    return out


def extend(args, torch):
    model = build_model(torch)
    out = {"root": os.path.abspath(args.root), "S": S, "repeats": args.repeats, "totals_ms": {}, "blocks": {}, "warmup_blocks": {},
           "last_label_max_abs_diff": {}}
    for B in (1, 8, 32):
        text, _ = inputs(torch, B)
        sess = model.stream(capacity=B)
        lengths = [S - 1] * B

        def steps():
            for u in range(S):
                lp = sess.step(text[u])
            return lp

        def chunk():
            sess.extend(text[:S - 1], lengths)
            return sess.step(text[S - 1])

        variants = {"steps": steps, "extend": chunk}

        def whole(name):
            sess.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lp = variants[name]()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, lp.clone()

        runs = {k: [] for k in variants}
        last = {}
        for r in range(args.repeats + WARMUP_ROUNDS):
            for k in variants:
                ms, last[k] = whole(k)
                runs[k].append(ms)
        out["last_label_max_abs_diff"]["B%d" % B] = float((last["steps"] - last["extend"]).abs().max())
        for k, vals in runs.items():
            key = "B%d_%s" % (B, k)
            out["blocks"][key] = [round(x, 3) for x in vals[WARMUP_ROUNDS:]]
            out["warmup_blocks"][key] = [round(x, 3) for x in vals[:WARMUP_ROUNDS]]
            out["totals_ms"][key] = summary(vals[WARMUP_ROUNDS:])
        del sess
    a_, b_ = out["totals_ms"]["B32_steps"], out["totals_ms"]["B32_extend"]
    margin = max(a_["spread"], b_["spread"])
    out["condition_B32"] = {"steps_median_ms": a_["median"], "extend_median_ms": b_["median"], "larger_spread_ms": margin,
                            "holds": bool(a_["median"] - b_["median"] > margin)}
    return out


def kernels(args, torch):
    from gan_ffn_amd import _lib, ops
    n = cap = 32
    max_len, m = 110, S - 1
    In, H, L = DIMS[0], DIMS[1], 4
    out = {"lib": _lib.LIB_PATH, "launches": args.launches, "repeats": args.repeats, "position": S - 1, "rows": n, "extend_m": m,
           "blocks": {}}
    torch.manual_seed(5)
    lstm = torch.nn.LSTM(In, H, num_layers=L, bidirectional=False).cuda().eval()
    cfg = ops.lstm_stream_cfg(cap, max_len, In, H, L)
    n_state, n_ws = ops.lstm_stream_sizes(cfg, n)
    g = torch.Generator().manual_seed(5)
    state = ((torch.rand(n_state, generator=g) - 0.5) * 0.6).cuda()
    ws = torch.empty(n_ws, device="cuda")
    x = (torch.rand(m, n, In, generator=g) - 0.5).cuda()
    slot = torch.arange(n, dtype=torch.int32, device="cuda")
    pos = torch.full((cap,), S - 1, dtype=torch.int32, device="cuda")
    pos0 = torch.zeros(cap, dtype=torch.int32, device="cuda")
    count = torch.full((n,), m, dtype=torch.int32, device="cuda")
    e_out = torch.empty(m, n, H, device="cuda")
    ptrs = ops.lstm_stream_ptrs(lstm)

    def step():       # every call rewrites the same state words (position 32 of every slot) from the state it left
        ops.lstm_stream_step_raw(cfg, n, slot, pos, x[0], ptrs, state, e_out[0], ws)

    def chunk():      # positions 0 .. 31 of every slot
        ops.lstm_stream_extend_raw(cfg, n, m, slot, count, pos0, x, ptrs, state, e_out, ws)

    for name, launch, calls in (("lstm_step_9_launches_us", step, args.launches),
                                ("lstm_extend_m32_us", chunk, max(1, args.launches // m))):
        launch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(calls):
                launch()
        runs = []
        for _ in range(args.repeats + 1):             # the first round is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            runs.append(round(e0.elapsed_time(e1) * 1e3 / calls, 3))
        out["blocks"][name] = runs[1:]
        out[name] = summary(runs[1:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--extend", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    print(json.dumps((kernels if args.kernels else extend if args.extend else sessions)(args, torch)), flush=True)


if __name__ == "__main__":
    main()
