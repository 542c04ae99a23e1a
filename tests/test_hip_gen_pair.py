"""The eval-mode and the train-mode forward of one generator as ONE two-segment encoder pass (ganffn_encoder_fwd_pair) against
the two ganffn_encoder_fwd calls it replaces, and GanEngine with the pairing on against GANFFN_GEN_PAIR=0 — bit for bit."""
import pytest
import torch

from test_hip_engine import build_all, gan_batch

pytestmark = pytest.mark.gpu

# (S, B): T = 14 is no multiple of 4 (a Philox row group of a joint [2 T] matrix would straddle the segments), 36 is a
# multiple of 4 but not of 16 (the row chain's tile), 64 is tile-aligned, 282 is the workload's S with every key tile in use
SHAPES = [(7, 2), (9, 4), (16, 4), (94, 3)]
# (E, H), L = 2: "LayerNorm2 carries the next in-proj" and the last-layer path both run.  (120, 4): 30-wide heads on the generic
# GEMM path (the 16-row attention kernels' third head shape); (64, 4) and (248, 4): head_dim 16 and 62 on the 32-row attention
# kernel's run-time head_dim form, whose two-segment instantiation no workload width reaches
WIDTHS = [(100, 10), (512, 8), (120, 4), (64, 4), (248, 4)]
# (S, B, E, H): four query tiles at B H >= 512 — the 16-row attention forward (head_dim 10 and 30) runs a batch as whole workgroups
# where the smaller launches above are cut in two, and the rule is that of ONE batch of B dialogues in the two-segment launch too
UNCUT = [(50, 52, 100, 10), (50, 128, 120, 4)]


def pair_cases(shapes):
    """every shape at every width, then UNCUT"""
    return [(S, B, E, H) for E, H in WIDTHS for S, B in shapes] + UNCUT


def _case(S, B, E, H, L=2, F=None):
    from gan_ffn_amd import ops
    F = ops.FF if F is None else F
    g = torch.Generator().manual_seed(1000 * S + 10 * B + E)
    cfg = ops.enc_cfg(S, B, E, H, L, F=F, train=True)
    cfg_eval = ops.enc_cfg(S, B, E, H, L, F=F, train=False)
    per, _ = ops.layer_layout(E, F)
    params = ((torch.rand(L * per, generator=g) - 0.5) * 0.2).cuda()
    x = torch.rand(S, B, E, generator=g).cuda()
    pe = torch.rand(S, E, generator=g).cuda()
    return cfg, cfg_eval, params, x, pe


def _pair_against_the_two_single_passes(S, B, E, H, mode=0, key_len=None, F=None):
    """mode: the debug mode word (ganffn_debug_set_ffn_mode) all three calls run under; key_len: handed to all three;
    F: the feed-forward width (None: the networks' 2048)"""
    from gan_ffn_amd import _lib, ops
    cfg, cfg_eval, params, x, pe = _case(S, B, E, H, F=F)
    n_saved, n_ws = ops.enc_sizes(cfg)
    ops.manual_seed(4321)
    rng, add = ops.DeviceRng.get("cuda").state, 17
    f32 = dict(device="cuda", dtype=torch.float32)
    # reference: eval unsaved, then train saved with the same offset; buffers start from the same fill on both sides, so the
    # WHOLE saved buffer compares (words no launch writes included)
    out_e, out_t = torch.zeros(S * B * E, **f32), torch.zeros(S * B * E, **f32)
    saved = torch.full((n_saved,), -7.0, **f32)
    ws = torch.zeros(n_ws, **f32)
    p_e, p_t = torch.zeros(S * B * E, **f32), torch.zeros(S * B * E, **f32)
    p_saved = torch.full((n_saved,), -7.0, **f32)
    p_ws = torch.zeros(ops.encoder_fwd_pair_workspace_floats(cfg), **f32)
    lib = _lib.load()
    lib.ganffn_debug_set_ffn_mode(mode)
    try:
        ops.encoder_fwd_raw(cfg_eval, x, pe, params, out_e, None, ws, rng, add, key_len=key_len)
        ops.encoder_fwd_raw(cfg, x, pe, params, out_t, saved, ws, rng, add, key_len=key_len)
        # every width here has its two-segment forms under these mode words (a width that lost them would have to be refused:
        # test_a_lab_variant_without_a_segment_form_is_reported_and_refused) — asserted, so that none drops out of this comparison
        assert ops.encoder_fwd_pair_supported(cfg)
        ops.encoder_fwd_pair_raw(cfg, x, pe, params, p_e, p_t, p_saved, p_ws, rng, add, key_len=key_len)
        torch.cuda.synchronize()
    finally:
        lib.ganffn_debug_set_ffn_mode(0)
    assert torch.isfinite(out_e).all() and torch.isfinite(out_t).all() and not torch.equal(out_e, out_t)
    assert torch.equal(p_e, out_e)
    assert torch.equal(p_t, out_t)
    assert torch.equal(p_saved.view(torch.int32), saved.view(torch.int32))


@pytest.mark.parametrize("S,B,E,H", pair_cases(SHAPES))
def test_pair_pass_equals_the_two_single_passes(S, B, E, H):
    _pair_against_the_two_single_passes(S, B, E, H)


# the smallest shapes that select the two-segment forms of the GEMM driver's special kernels (csrc/gemm.hip gemm_plan), d_model 100:
#   T = 70, F = 1024: linear1 [70 x 100] -> 1024 on the weight-resident kernel's pair form (K = 100, N >= 1024; two token tiles
#     per segment, the second with 6 rows), linear2 (K = 1024) on gemm_n100's pair form
#   T = 17, F = 256: linear2 at gemm_n100's smallest K, one ragged token tile per segment; linear1 (N = 256 < 1024) on the
#     short-K pair form of the generic kernel
#   d_model 64, F = 128 / 132: linear1's K = 64 on the short-K pair forms of both epilogues, linear2's K on either side of the
#     short-K threshold of the plain pair form
@pytest.mark.parametrize("S,B,E,H,F", [(35, 2, 100, 10, 1024), (17, 1, 100, 10, 256), (17, 1, 64, 4, 128), (17, 1, 64, 4, 132)])
def test_pair_pass_equals_the_two_single_passes_at_the_thresholds_of_the_gemm_plan(S, B, E, H, F):
    _pair_against_the_two_single_passes(S, B, E, H, F=F)


# the older launch sequences of the mode word (include/ganffn.h: bit 1 separate GEMM + LayerNorm launches, bit 2 generic tiles
# for the 2048 -> 100 product, bit 6 PE and layer 0's in-proj as two launches, bit 24 the wide out-proj unsplit), each at the
# width whose walk it changes; mode 0 at 512 is the split out-proj that bit 24 turns off
OLDER_SEQUENCES = [(2, 100, 10), (4, 100, 10), (6, 100, 10), (64, 100, 10), (2 | 64, 100, 10), (1 << 24, 512, 8), (0, 512, 8)]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("mode,E,H", OLDER_SEQUENCES)
@pytest.mark.parametrize("S,B", [(7, 2), (9, 4)])
def test_pair_pass_equals_the_two_single_passes_under_older_launch_sequences(S, B, mode, E, H, ragged):
    """the pair pass and the two single passes take the same branches of the one forward walk.  T = 14: a Philox row group of a
    joint [2 T] matrix would straddle the segments; T = 36: gemm_splitk_factor gives 8 slabs for the 2048 -> 100 product and 2
    for the 512-wide out-proj, so the split and the unsplit out-proj differ.  ragged: key lengths [S, 1] / [S, 1, S // 2, 2]
    through the _len entry points."""
    key_len = torch.tensor([S, 1, S // 2, 2][:B], dtype=torch.int32, device="cuda") if ragged else None
    _pair_against_the_two_single_passes(S, B, E, H, mode, key_len)


def test_a_lab_variant_without_a_segment_form_is_reported_and_refused():
    """every width has its segment forms (WIDTHS above: row chain + 16-row attention; generic GEMMs + 16-row attention at
    S <= 48 / the 32-row kernel above; 30-wide heads) — only a lab variant of the 2048 -> 100 product selected through the debug
    mode word has none: _supported answers 0 and the entry point fails instead of computing something else"""
    from gan_ffn_amd import _lib, ops
    S, B, E, H = 9, 4, 100, 10
    cfg, _, params, x, pe = _case(S, B, E, H)
    assert ops.encoder_fwd_pair_supported(cfg)
    n_saved, n_ws = ops.enc_sizes(cfg)
    f32 = dict(device="cuda", dtype=torch.float32)
    out_e, out_t = torch.zeros(S * B * E, **f32), torch.zeros(S * B * E, **f32)
    saved = torch.zeros(n_saved, **f32)
    ws = torch.zeros(max(n_ws, ops.encoder_fwd_pair_workspace_floats(cfg)), **f32)
    lib = _lib.load()
    lib.ganffn_debug_set_ffn_mode(1 << 23)          # the padded seventh tile instead of the 4x4x1 tail
    try:
        assert not ops.encoder_fwd_pair_supported(cfg)
        with pytest.raises(_lib.GanffnError):
            ops.encoder_fwd_pair_raw(cfg, x, pe, params, out_e, out_t, saved, ws, ops.DeviceRng.get("cuda").state, 0)
    finally:
        lib.ganffn_debug_set_ffn_mode(0)
    torch.cuda.synchronize()
    assert not out_e.any() and not out_t.any() and not saved.any()


def _run_engine(S, B, n_streams, use_graph, pair, monkeypatch, iters=2):
    """pair: "all" = every (D, G) sub-step pair whose generator has a pair pass, "1" = those that gained from it, "0" = none,
    None = GANFFN_GEN_PAIR unset: 1 in the multi-stream runner, 0 on one stream"""
    from gan_ffn_amd import engine, ops
    if pair is None:
        monkeypatch.delenv("GANFFN_GEN_PAIR", raising=False)
        pair = "1" if n_streams > 1 else "0"
    else:
        monkeypatch.setenv("GANFFN_GEN_PAIR", pair)
    gens, discs = build_all(zero_dropout=False)
    ops.manual_seed(99)
    eng = engine.GanEngine(gens, discs, n_streams=n_streams, use_graph=use_graph)
    assert eng.gen_pair == (pair != "0") and eng.gen_pair_mode == pair
    batch = gan_batch(S=S, B=B)
    losses = []
    for _ in range(iters):
        ls = eng.iteration(batch)
        eng.synchronize()
        losses.append(ls.clone())
    torch.cuda.synchronize()
    # every (D, G) sub-step pair of the reference schedule is on one stream and has a pair pass; by default the two of the
    # 512-wide visual generator are taken (engine.GEN_PAIR_MAX_UNPAIRED_E)
    paired = [i for i in range(12) if eng._pair_slot(i) is not None]
    assert paired == {"all": [0, 2, 4, 6, 8, 10], "1": [8, 10], "0": []}[pair], paired
    state = {}
    for grp, nets in (("G", eng.G), ("D", eng.D)):
        for k, st in nets.items():
            for name in ("slab", "grad", "exp_avg", "exp_avg_sq"):
                state[(grp, k, name)] = getattr(st, name).detach().clone()
    return torch.stack(losses), state


def _compare(a, b):
    assert torch.isfinite(a[0]).all() and a[0].shape == (2, 12)
    assert torch.equal(a[0], b[0]), (a[0] - b[0]).abs().max()
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("S,B", [(9, 4), (94, 4)])
def test_engine_with_pairing_equals_engine_without(S, B, n_streams, monkeypatch):
    on = _run_engine(S, B, n_streams, False, "all", monkeypatch)
    off = _run_engine(S, B, n_streams, False, "0", monkeypatch)
    _compare(on, off)


def test_engine_with_default_pairing_equals_engine_without(monkeypatch):
    on = _run_engine(9, 4, 3, False, None, monkeypatch)          # three streams, nothing set: the 512-wide generator's two pairs
    off = _run_engine(9, 4, 3, False, "0", monkeypatch)
    _compare(on, off)
    one = _run_engine(9, 4, 1, False, "1", monkeypatch)          # the same choice asked for on one stream
    _compare(one, _run_engine(9, 4, 1, False, None, monkeypatch))    # ... against one stream's default: unpaired
    _compare(one, off)


def test_engine_with_pairing_equals_engine_without_under_graph_replay(monkeypatch):
    on = _run_engine(9, 4, 1, True, "all", monkeypatch)
    off = _run_engine(9, 4, 1, True, "0", monkeypatch)
    _compare(on, off)
