"""Case tables, seeded inputs, the range runner and the oracle evaluations of tests/test_hip_encoder_ranges.py (GPU) and
tests/test_encoder_range_cases_cpu.py (no GPU).

The inputs are tests/test_hip_dispatch_range.py's (_encoder_inputs / _encoder_params: seeded slab, x, pe, d_out); the expected
values are oracle.ganffn_oracle.encoder_stack in fp64 with the contract's Philox masks (seed ENC_SEED, offset ENC_ADD) and,
on the GPU, the ReLU pattern the HIP forward took.  The yardstick of every bound is the same oracle in fp32 on the CPU."""
import contextlib
import ctypes as C
import types

import numpy as np
import torch

import key_len_oracle as KO
from oracle import ganffn_oracle as O
from oracle import philox
from test_hip_dispatch_range import ENC_ADD, ENC_SEED, _encoder_inputs, _encoder_params

# ------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------
ROWCHAIN, WORKLOAD, GENERIC = (100, 10, 2048), (512, 8, 2048), (64, 4, 128)      # (E, H, F)
WIDTHS = [ROWCHAIN, WORKLOAD, GENERIC]
SHAPES = [(9, 4), (33, 3)]                                                        # (S, B)

# L -> partitions of [0, L) in call order (top range first)
PARTITIONS = {
    4: [((2, 4), (0, 2)), ((3, 4), (1, 3), (0, 1)), ((3, 4), (2, 3), (1, 2), (0, 1))],
    8: [((5, 8), (2, 5), (0, 2))],                     # GanEngine's gradient buckets at n_buckets = 3
}

# the tolerances of test_encoder_stack_matches_oracle_off_the_workload_widths: quantity -> (rtol, atol)
EXISTING = {"out": (1e-4, 1e-6), "dx": (2e-4, 1e-8), "grad": (1e-3, 1e-8)}


def case(width, L, S, B, train=True, lengths=None):
    E, H, F = width
    return types.SimpleNamespace(E=E, H=H, F=F, L=L, S=S, B=B, train=train, lengths=lengths)


def case_id(c):
    return "E%d-L%d-%dx%d-%s%s" % (c.E, c.L, c.S, c.B, "train" if c.train else "eval", "-len" if c.lengths is not None else "")


def ranges_id(r):
    return "".join("[%d,%d)" % ab for ab in r)


# (case, partition): every partition at every width and shape in train mode, one case at T = 564 where a two-layer tn100
# group cuts its token range in two, one eval-mode case per width
RANGE_CASES = [(case(w, L, S, B), p) for w in WIDTHS for (S, B) in SHAPES for L in sorted(PARTITIONS) for p in PARTITIONS[L]]
RANGE_CASES += [(case(ROWCHAIN, 4, 94, 6), PARTITIONS[4][0])]
RANGE_CASES += [(case(w, 4, 9, 4, train=False), PARTITIONS[4][1]) for w in WIDTHS]

# key lengths over (S, B) = (9, 4): a dialogue of one utterance, a full one, two in between
LEN_CASE = (case(ROWCHAIN, 4, 9, 4, lengths=(1, 9, 4, 7)), PARTITIONS[4][0])
LEN_CASES = [LEN_CASE, (case(GENERIC, 4, 9, 4, lengths=(1, 9, 4, 7)), PARTITIONS[4][0])]

# deep stacks, (S, B) = (5, 2).  d_model 100: 4 L weight-gradient problems against the 40 of one grouped launch (10: one full
# launch; 11: 40 + 4; 21: 40 + 40 + 4), 2 L LayerNorm instances against the 32 of one reduce launch (16 | 17).  64 wide: the
# generic grouped kernel on the same counts, and L = 64, the limit of check_cfg, which fills the host arrays of the reduce
DEEP_S, DEEP_B = 5, 2
DEEP_L = {ROWCHAIN: [10, 11, 16, 17, 21], GENERIC: [11, 17, 64]}
DEEP_CASES = [case(w, L, DEEP_S, DEEP_B) for w in (ROWCHAIN, GENERIC) for L in DEEP_L[w]]
DEEP_EVAL_CASES = [case(w, 17, DEEP_S, DEEP_B, train=False) for w in (ROWCHAIN, GENERIC)]
GROUP_PROBLEMS, LN_REDUCE_INSTANCES, MAX_LAYERS = 40, 32, 64


def tiles_top_down(L, ranges):
    """the ranges cover [0, L) exactly once, top range first"""
    hi = L
    for lo_, hi_ in ranges:
        if not (0 <= lo_ < hi_ == hi):
            return False
        hi = lo_
    return hi == 0


# ------------------------------------------------------------------------------------------------------------------------
# unreduced chunk slabs: the chunk count of gemm_tn100.hip's grouped launch, restated
# ------------------------------------------------------------------------------------------------------------------------
TN100_TILES_PER_LAYER = 32 + 32 + 2 + 5            # 64-wide tiles of the long side: linear2, linear1, out-proj (100), in-proj (300)
TN100_TARGET, TN100_MAX_CHUNKS, TN100_MIN_TOKENS = 1700, 8, 256
PART_FLOATS = (2560 + 256) * (64 * 64 + 64) + 4 * 40      # ganffn_gemm_tn_grouped_workspace_floats()
LAYER_FLOATS_100 = 452548                                  # ganffn_layer_param_count(100, 2048)
COVERED_100 = 452148                                       # ganffn_encoder_bwd_parts_covered(100, 2048): the four weights and biases


def expected_chunks(L, T, part_floats=PART_FLOATS, layer_floats=LAYER_FLOATS_100, covered=COVERED_100):
    """-> (n_parts of ganffn_encoder_bwd_parts for an L-layer (100, 10, 2048) stack over T tokens, the binding term): the
    load target ceil(1700 / tiles) | the cap 8 | 256 tokens per workgroup | the reduce launch's workspace (one slab of all
    weight gradients and bias sums per chunk: its count is the unreduced form's too, or the two would associate the sum
    differently) | the unreduced form's own workspace (one gradient-shaped slab per chunk beyond the first)"""
    tiles = TN100_TILES_PER_LAYER * L
    terms = {"target": -(-TN100_TARGET // tiles), "cap": TN100_MAX_CHUNKS, "tokens": T // TN100_MIN_TOKENS,
             "reduce workspace": part_floats // (L * covered), "slab workspace": 1 + part_floats // (L * layer_floats)}
    n = min(terms.values())
    binding = [k for k in terms if terms[k] == n][0]
    return max(n, 1), binding


# (L, S, B) -> T = 320, 564, 1100
SLAB_SHAPES = [(40, 8), (94, 6), (110, 10)]
SLAB_CASES = [(L, S, B) for L in (1, 2, 10) for (S, B) in SLAB_SHAPES] + [(8, 110, 10)]      # (the workload's depth: 3 chunks)
# what the rule gives, written out: L = 1, 2 stop at 256 tokens per workgroup (1, 2, 4 chunks).  At L = 10 and T = 1100 the load
# target asks for 3 chunks and the WORKSPACE is what binds: 3 slabs of the reduce launch (3 x 4521480 floats) do not fit into
# 11714720, so both forms run 2 chunks.  (The unreduced form alone would fit 3 — 2 gradient-shaped slabs — and ran 3 until
# this test was written: its Adam step then had other bits than the reduce launch's.)
SLAB_CHUNKS = {(1, 320): 1, (1, 564): 2, (1, 1100): 4, (2, 320): 1, (2, 564): 2, (2, 1100): 4,
               (10, 320): 1, (10, 564): 2, (10, 1100): 2, (8, 1100): 3}


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def inputs(c):
    """-> (slab, x, pe, d_out) of _encoder_inputs, with 1 added to every LayerNorm weight.  The seeded slab draws ALL
    parameters from +-0.1, the LayerNorm weights too, and each layer then shrinks the gradient that passes through it about
    tenfold: in the fp64 oracle layer 0 of an 8-layer stack has gradients of 1e-4 against 10 in layer 7, of a 21-layer stack
    1e-12, of a 64-layer stack 1e-36 — below any tolerance and below the seeded initial gradient values, so a wrong lower
    layer could not show.  With weights around 1 every layer's gradients are of order 10 at every depth here."""
    from gan_ffn_amd import ops
    slab, x, pe, dout = _encoder_inputs(c.S, c.B, c.E, c.H, c.F, c.L)
    per, offs = ops.layer_layout(c.E, c.F)
    for l in range(c.L):
        for o in (offs[8], offs[10]):
            slab[l * per + o:l * per + o + c.E] += 1.0
    return slab, x, pe, dout


def seeded_gradients(n, seed=7):
    """a non-zero gradient slab for the backward to add to: uniform in +-0.05, no element 0"""
    g = torch.Generator().manual_seed(seed + n)
    t = (torch.rand(n, generator=g) - 0.5) * 0.1
    return torch.where(t == 0, torch.full_like(t, 0.01), t)


def keys(L):
    from gan_ffn_amd import ops
    return ["transformer_encoder.layers.%d.%s" % (l, k) for l in range(L) for k in ops.LAYER_KEYS]


def slab_views(slab, E, F, L):
    """key -> view of a [L x layer] slab"""
    from gan_ffn_amd import ops
    per, offs = ops.layer_layout(E, F)
    out = {}
    for l in range(L):
        for key, o, shape in zip(ops.LAYER_KEYS, offs, ops.layer_shapes(E, F)):
            out["transformer_encoder.layers.%d.%s" % (l, key)] = slab[l * per + o:l * per + o + int(np.prod(shape))].view(shape)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# oracle
# ------------------------------------------------------------------------------------------------------------------------
def oracle_eval(c, ins, masks=None, dtype=torch.float64):
    """O.encoder_stack and the backward of the seeded d_out in `dtype` -> namespace(out, dx, grads by key, trace, masks);
    masks: the per-layer ReLU patterns (S, B, F) to run on, None = the evaluation's own (returned as .masks)"""
    slab, x, pe, dout = ins
    P = _encoder_params(slab, pe, c.E, c.F, c.L)
    if dtype != torch.float64:
        P = {k: (v.detach().to(dtype).requires_grad_(True) if v.requires_grad else v.to(dtype)) for k, v in P.items()}
    xo = x.to(dtype).requires_grad_(True)
    trace = []
    rng = O.Rng(ENC_SEED, ENC_ADD, True) if c.train else None
    ctx = KO.masked_attention(c.lengths) if c.lengths is not None else contextlib.nullcontext()
    with ctx:
        yo = O.encoder_stack(xo, P, c.H, rng, n_layers=c.L, relu_masks=None if masks is None else [m.to(dtype) for m in masks],
                             trace=trace)
        (yo * dout.to(dtype)).sum().backward()
    own = [(t > 0).double() for t in trace]
    return types.SimpleNamespace(out=yo.detach().double(), dx=xo.grad.double(), grads={k: P[k].grad.double() for k in keys(c.L)},
                                 trace=trace, masks=own if masks is None else masks)


def expected(c, ins, g0, masks=None):
    """-> (r64, r32): the fp64 and fp32 oracle on one ReLU pattern (None: the fp64 evaluation's own), with the parameter
    gradients as the slab reads after the backward: initial value + gradient (the fp32 one added in fp32)"""
    r64 = oracle_eval(c, ins, masks)
    r32 = oracle_eval(c, ins, r64.masks, torch.float32)
    v0 = slab_views(g0, c.E, c.F, c.L)
    r64.grads = {k: v0[k].double() + g for k, g in r64.grads.items()}
    r32.grads = {k: (v0[k] + g.float()).double() for k, g in r32.grads.items()}
    return r64, r32


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def bound(kind, fp32_err):
    """rtol of a check: max(the project's tolerance, 8 x the fp32 oracle's error) — _range_bound"""
    from test_hip_dispatch_range import _range_bound
    return _range_bound(EXISTING[kind][0], fp32_err)


def quantities(r, L):
    """(kind, label, tensor) of everything a case compares"""
    yield "out", "out", r.out
    yield "dx", "dx", r.dx
    for k in keys(L):
        yield "grad", "grad " + k, r.grads[k]


# ------------------------------------------------------------------------------------------------------------------------
# GPU side
# ------------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def forward(c, ins=None):
    """one ganffn_encoder_fwd (or _fwd_len) with `saved` -> everything the backward calls need, the output and the ReLU
    patterns on the host"""
    from gan_ffn_amd import ops
    slab, x, pe, dout = ins = ins if ins is not None else inputs(c)
    cfg = ops.enc_cfg(c.S, c.B, c.E, c.H, c.L, F=c.F, train=c.train)
    n_saved, n_ws = ops.enc_sizes(cfg)
    f32 = dict(device="cuda", dtype=torch.float32)
    fw = types.SimpleNamespace(c=c, ins=ins, cfg=cfg, n_ws=n_ws, slab_d=slab.cuda(), dout_d=dout.cuda().contiguous(),
                               rng=torch.tensor([ENC_SEED, 0], dtype=torch.int64, device="cuda"),
                               key_len=None if c.lengths is None else torch.tensor(c.lengths, dtype=torch.int32, device="cuda"))
    out = torch.full((c.S * c.B * c.E,), float("nan"), **f32)
    fw.saved, fw.ws = torch.zeros(n_saved, **f32), torch.full((n_ws,), float("nan"), **f32)
    fw.x_d, fw.pe_d = x.cuda(), pe.cuda()
    ops.encoder_fwd_raw(cfg, fw.x_d, fw.pe_d, fw.slab_d, out, fw.saved, fw.ws, fw.rng, ENC_ADD, key_len=fw.key_len)
    torch.cuda.synchronize()
    fw.out = out.view(c.S, c.B, c.E).cpu()
    fw.masks = []
    n = c.S * c.B * c.F
    for l in range(c.L):
        off = int(ops._lib.load().ganffn_encoder_saved_hidden_offset(C.byref(cfg), l))
        assert off >= 0 and off + n <= n_saved
        fw.masks.append((fw.saved[off:off + n] != 0).view(c.S, c.B, c.F).double().cpu())     # dropped units read 0: gradient 0 whatever the pattern
    return fw


def run_ranges(fw, ranges, g0=None, grads=True, need_dx_in=True):
    """the backward of the seeded d_out as one ganffn_encoder_bwd2 (_bwd_len) call per range, in the order given, on one dx
    buffer and one gradient slab that starts as g0 (grads=False: NULL is passed).  The workspace is refilled with NaN before
    every call: it is scratch, no call may read what an earlier one left there -> (dx, gradient slab) on the host"""
    from gan_ffn_amd import ops
    dx = fw.dout_d.clone()
    gslab = None if not grads else (torch.zeros_like(fw.slab_d) if g0 is None else g0.cuda())
    for lo, hi in ranges:
        fw.ws.fill_(float("nan"))
        ops.encoder_bwd_raw(fw.cfg, lo, hi, dx, fw.slab_d, gslab, fw.saved, fw.ws, fw.rng, ENC_ADD, need_dx_in, key_len=fw.key_len)
    torch.cuda.synchronize()
    return dx.cpu(), None if gslab is None else gslab.cpu()


def kink_flips(c, fw, r64):
    """the audit that licenses running the oracle on the HIP pattern: every unit the contract drops reads 0, and a kept unit
    whose pattern differs from the oracle's own has an fp64 pre-activation within 2e-5 of the layer's scale -> flips"""
    flips = 0
    p = O.ENC_DROPOUT if c.train else 0.0
    for l in range(c.L):
        kept = torch.from_numpy(philox.keep_mask(c.S * c.B, c.F, p, O.SITE_LAYER0 + 4 * l + 2, ENC_SEED, ENC_ADD)).view(c.S, c.B, c.F)
        assert not bool((fw.masks[l] > 0)[~kept].any())
        diff = kept & ((r64.trace[l] > 0) != (fw.masks[l] > 0))
        flips += int(diff.sum())
        if diff.any():
            assert float(r64.trace[l][diff].abs().max()) < 2e-5 * max(1.0, float(r64.trace[l].abs().max())), (l, float(r64.trace[l][diff].abs().max()))
    return flips
