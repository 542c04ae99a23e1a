"""The per-step emotion cell of the HIP DialogueRNN (csrc/dialogue_rnn.hip: D_e > 128, where drnn_echain_fwd / _bwd_kernel do
not apply) and the limits check_drnn / check_att accept, against the fp64 torch restatement on the CPU: emotions, every alpha,
dU and every parameter gradient (tests/test_hip_drnn_kernel.py's compare and its tolerances, e 2e-5 and gradients 3e-4 of the
largest reference entry).

Widths (D_m, D_g = D_p, D_e): (8, 128, 128) is the widest emotion chain, (8, 136, 132) the per-step cell just past the switch
with D_e <= D_g, (8, 64, 132) the per-step cell with D_e > 2 D_g: its pre-activations [B x 3 D_e] and its direct-path gradient
[B x D_e] then need the workspace regions GI, GH and dhdir sized for D_e (a layout that sizes them for D_g lets the two products
of the emotion cell's launch write the same floats: GH starts 3 B D_g floats behind GI, which is 3 B D_e long).  Every width
runs eval, train with the same Philox masks (the emotion site's mask is [S B x D_e]), the listener (QN then comes from the
listener kernel), three parties, two directions in one call (the per-step products sit at 2z and 2z + 1 of their launch), S = 1
(the first step is the last) and 33 dialogues (two dialogue tiles, the batch entry points).

Each test counts the native calls (one forward, one backward, at the expected D_e and B): a module that fell back to the
per-step torch cell would pass every comparison.

Tolerances: compare's own; no width needed more, so the 8 x (fp32 against fp64 on the CPU) rule of test_hip_dispatch_range.py was
not applied.  Largest error / tolerance measured on an MI355X over the seven cases of a width, for e, dU and the worst
parameter gradient: (8, 128, 128) 0.010, 0.002, 0.005; (8, 136, 132) 0.009, 0.002, 0.008; (8, 64, 132) 0.010, 0.001, 0.003;
the limits group 0.020 (S = 112), 0.001, 0.011 (concat, D_a = 512).  The same modules in fp32 against fp64 on the CPU differ
by about 2e-7 in e and 1e-6 in the gradients (0.01 and 0.003 of the tolerances): the kernels sit at fp32 rounding.  Each
test prints its figures (pytest -s)."""
import copy

import pytest
import torch

import test_hip_drnn_kernel as K
import test_hip_drnn_parties as PT
from test_hip_drnn_kernel import _MaskSeq, compare, philox_masks

pytestmark = pytest.mark.gpu

WIDTHS = [(8, 128, 128), (8, 136, 132), (8, 64, 132)]
# case -> (S, B, parties, listener, train, directions)
CASES = {"eval": (5, 3, 2, False, False, 1), "train": (5, 3, 2, False, True, 1), "listener": (5, 3, 2, True, False, 1),
         "three-parties": (5, 3, 3, False, False, 1), "two-directions": (5, 3, 2, False, False, 2), "one-step": (1, 2, 2, False, False, 1),
         "two-tiles": (3, 33, 2, False, False, 1)}
P_DROP, SEED = 0.1, 20261020


def model(dims, att="general", listener=False, D_a=100, seed=7, dropout=P_DROP):
    """test_hip_drnn_kernel.build with the attention type, D_a and the listener open (the same seed and the same livelier weights)"""
    from gan_ffn_amd import dialogue_rnn as DR
    if att == "general" and not listener:
        return K.build(seed=seed, dropout=dropout, dims=dims)
    torch.manual_seed(seed)
    m = DR.DialogueRNN(context_attention=att, listener_state=listener, D_a=D_a, dropout=dropout, **dims)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)
    return m


def inputs(S, B, P, seed, Dm):
    U, qmask = K.make_inputs(S, B, seed, Dm=Dm) if P == 2 else PT.make_inputs(S, B, P, seed, Dm=Dm)
    assert qmask.shape == (S, B, P)
    return U, qmask


class _Pair(torch.nn.Module):
    """two DialogueRNNs as the two directions of ONE native call on the GPU (ops.dialogue_rnn_run with two cells), as two
    modules on the CPU; U holds both inputs side by side, the emotions come back side by side, alpha_t one under the other"""

    def __init__(self, a, b):
        super().__init__()
        self.a, self.b = a, b

    def forward(self, U, qmask):
        from gan_ffn_amd import ops
        Dm = U.size(2) // 2
        Us = [U[..., :Dm], U[..., Dm:]]
        if U.is_cuda:
            (e0, a0), (e1, a1) = ops.dialogue_rnn_run([self.a.dialogue_cell, self.b.dialogue_cell], Us, [qmask, qmask], self.training)
        else:
            (e0, a0), (e1, a1) = self.a(Us[0], qmask), self.b(Us[1], qmask)
        return torch.cat([e0, e1], 2), [torch.cat([x, y], 0) for x, y in zip(a0, a1)]


@pytest.fixture
def native_calls(monkeypatch):
    """[(what, B, D_e, parties, listener, directions)] of every ops.drnn_fwd_raw / drnn_bwd_raw call"""
    from gan_ffn_amd import ops
    seen = []
    fwd, bwd = ops.drnn_fwd_raw, ops.drnn_bwd_raw

    def counted(what, fn, i_lp):
        def call(cfg, acfg, parties, ndir, *rest):
            seen.append((what, cfg.B, cfg.He, parties, rest[i_lp] is not None, ndir))
            return fn(cfg, acfg, parties, ndir, *rest)
        return call
    monkeypatch.setattr(ops, "drnn_fwd_raw", counted("fwd", fwd, 4))      # rest: U spk mval P LP ...
    monkeypatch.setattr(ops, "drnn_bwd_raw", counted("bwd", bwd, 5))      # rest: d_e U spk mval P LP ...
    return seen


def check(m_cpu, U, qmask, native_calls, tag, directions=1, masks=None):
    """compare() on a GPU copy of m_cpu, with the proof that the HIP recurrence produced what was compared"""
    from gan_ffn_amd import ops
    m_gpu = copy.deepcopy(m_cpu).float().cuda()
    cells = [m_gpu.dialogue_cell] if directions == 1 else [m_gpu.a.dialogue_cell, m_gpu.b.dialogue_cell]
    S, B, P = qmask.shape
    for cell in cells:
        pred = ops.dialogue_rnn_listener_supported if cell.listener_state else ops.dialogue_rnn_supported
        assert pred(cell, U.cuda()[..., :cell.D_m], qmask.cuda())
    if masks is not None:
        m_cpu.dialogue_cell.dropout = _MaskSeq(masks)
        ops.manual_seed(SEED)                       # the call below takes rng offset 0
    figures = {}
    try:
        compare(m_gpu, m_cpu, U, qmask, figures=figures)
    finally:
        print("%s: error / tolerance %s" % (tag, " ".join("%s %.3f" % kv for kv in sorted(figures.items()))))
    call = (B, cells[0].D_e, P, bool(cells[0].listener_state), directions)
    assert native_calls == [("fwd",) + call, ("bwd",) + call]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("Dm,H,He", WIDTHS, ids=["%d-%d-%d" % w for w in WIDTHS])
def test_emotion_cell_on_both_sides_of_the_chain_limit(Dm, H, He, case, native_calls):
    S, B, P, listener, train, directions = CASES[case]
    dims = dict(D_m=Dm, D_g=H, D_p=H, D_e=He)
    U, qmask = inputs(S, B, P, seed=100 * S + B + P, Dm=Dm)
    if (S, B) == (5, 3):
        assert bool((qmask.sum(2) == 0).any()), "a ragged tail"
    mode = (lambda m: m.double().train()) if train else (lambda m: m.double().eval())
    masks = philox_masks(S, B, H, He, P_DROP, SEED, 0) if train else None
    if directions == 2:
        U = torch.cat([U, inputs(S, B, P, seed=77, Dm=Dm)[0] * (qmask.sum(2, keepdim=True) > 0)], 2)
        m_cpu = mode(_Pair(model(dims, seed=7), model(dims, seed=8)))
    else:
        m_cpu = mode(model(dims, listener=listener))
    check(m_cpu, U, qmask, native_calls, "(%d, %d, %d) %s" % (Dm, H, He, case), directions, masks)


# the limits check_drnn and check_att accept: (D_m, D_g = D_p, D_e), S, B, attention, D_a — the narrowest widths, the widest
# D_g the attention kernels take, DR_MAXS steps, concat attention at both ends of D_a
LIMITS = {"narrowest": ((4, 4, 4), 5, 3, "general", 100), "widest-D_g": ((8, 512, 4), 3, 2, "general", 100),
          "most-steps": ((8, 64, 4), 112, 2, "general", 100), "concat-D_a-4": ((8, 64, 4), 5, 3, "concat", 4),
          "concat-D_a-512": ((8, 64, 4), 5, 3, "concat", 512)}


@pytest.mark.parametrize("name", list(LIMITS))
def test_limits_the_checks_accept(name, native_calls):
    (Dm, H, He), S, B, att, D_a = LIMITS[name]
    U, qmask = inputs(S, B, 2, seed=100 * S + B, Dm=Dm)
    m_cpu = model(dict(D_m=Dm, D_g=H, D_p=H, D_e=He), att=att, D_a=D_a).double().eval()
    if att == "concat":
        assert m_cpu.dialogue_cell.attention.transform.weight.shape == (D_a, H + Dm)
    check(m_cpu, U, qmask, native_calls, name)
