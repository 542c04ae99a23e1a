"""Which gradients ganffn_drnn_att_bwd writes when only some gradient pointers are given: the input gradient and the
gradients that are asked for have the bits of a full backward, and a buffer that is not asked for is not touched.  One
direction, general and concat attention, eval and train mode; every output buffer starts from a fixed bit pattern."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

S, B, DM, H, HE, DA = 5, 3, 8, 8, 8, 8
PATTERN = 0x7FA5C3E1          # a NaN payload no kernel produces
ATT_SHAPES = {"general": [("w", (H, DM))], "concat": [("w", (DA, H + DM)), ("v", (1, DA))]}


def _pattern(*shape):
    return torch.full(shape, PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == PATTERN).all())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class _Run:
    def __init__(self, att, train):
        from gan_ffn_amd import _lib, ops
        self.ops, self.lib, self.att = ops, _lib, att
        g = torch.Generator().manual_seed(11)
        rnd = lambda *s: (torch.rand(*s, generator=g) - 0.5).cuda()
        self.cell = [rnd(3 * H, DM + H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H), rnd(3 * H, DM + H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H),
                     rnd(3 * HE, H), rnd(3 * HE, HE), rnd(3 * HE), rnd(3 * HE)]
        self.aprm = [rnd(*shape) for _, shape in ATT_SHAPES[att]]
        self.U, self.d_e = rnd(S, B, DM), rnd(S, B, HE)
        self.spk = torch.randint(0, 2, (S, B), generator=g).to(torch.int32).cuda()
        mval = torch.ones(S, B)
        mval[3:, 1] = 0                     # a padded tail
        self.mval = mval.cuda()
        self.cfg = _lib.DrnnCfg(S, B, DM, H, HE, 0.1, 1 if train else 0)
        self.acfg = _lib.DrnnAtt(_lib.DRNN_ATT_TYPES[att], DA if att == "concat" else 0)
        lib = _lib.load()
        n_saved = int(lib.ganffn_drnn_att_saved_floats(C.byref(self.cfg), C.byref(self.acfg), 0))
        n_ws = int(lib.ganffn_drnn_att_workspace_floats(C.byref(self.cfg), C.byref(self.acfg), 0))
        assert n_saved > 0 and n_ws > 0
        self.saved, self.ws = _pattern(n_saved), _pattern(n_ws)
        self.e, self.alpha = _pattern(S, B, HE), _pattern(B, S, S)
        self.rng = torch.tensor([20261020, 0], dtype=torch.int64, device="cuda")
        self._call("ganffn_drnn_att_fwd", [self.U], [self.spk], [self.mval], self._P(self.cell + [None]), None, self._AP(self.aprm),
                   [self.e], [self.alpha], [self.saved], [self.ws])

    def _P(self, tensors):
        return self.ops._ptr_structs(self.lib.DrnnPtrs, [tensors])

    def _AP(self, tensors):
        return self.ops._ptr_structs(self.lib.DrnnAttPtrs, [tensors], lambda a, _: self.ops._att_ptrs(self.att, a))

    def _call(self, name, *args):
        arr = lambda a: self.ops._ptr_array(a) if isinstance(a, list) else a
        self.lib.call(name, C.byref(self.cfg), C.byref(self.acfg), 1, *[arr(a) for a in args], self.ops._ptr(self.rng), C.c_uint64(3),
                      self.ops._stream())
        torch.cuda.synchronize()

    def backward(self, grads, agrads):
        """grads: 12 cell gradient tensors or None entries; agrads: the type's gradient tensors or None entries, or None for
        a null agrads argument.  Returns dU (written into a pattern-filled buffer)."""
        dU = _pattern(S, B, DM)
        self.ignored = _pattern(H, DM)      # grads.att_w: the att entry points ignore it (the weight's gradient is agrads.w)
        self._call("ganffn_drnn_att_bwd", [self.d_e], [self.U], [self.spk], [self.mval], self._P(self.cell + [None]), None,
                   self._AP(self.aprm), self._P(grads + [self.ignored]), None, self._AP(agrads) if agrads is not None else None, [dU],
                   [self.alpha], [self.saved], [self.ws])
        assert _untouched(self.ignored)
        return dU

    def zeros(self):
        return [torch.zeros_like(p) for p in self.cell], [torch.zeros_like(p) for p in self.aprm]

    def patterns(self):
        return [_pattern(*p.shape) for p in self.cell], [_pattern(*p.shape) for p in self.aprm]


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("att", ["general", "concat"])
def test_gradient_pointer_subsets(att, train):
    r = _Run(att, train)
    g_ref, ag_ref = r.zeros()
    dU_ref = r.backward(g_ref, ag_ref)
    assert bool(torch.isfinite(dU_ref).all()) and all(bool(g.abs().sum() > 0) for g in g_ref + ag_ref)
    none12 = [None] * 12

    # no gradient pointer at all (agrads null, or given with null members): the input gradient alone
    for agrads in (None, [None] * len(ag_ref)):
        g, ag = r.patterns()
        assert _same_bits(r.backward(none12, agrads), dU_ref)
        assert all(_untouched(t) for t in g + ag)

    # cell gradients without the attention weight's: the same cell gradients (and concat's v gradient)
    g, ag = r.zeros()
    assert _same_bits(r.backward(g, [None] + ag[1:]), dU_ref)
    assert all(_same_bits(a, b) for a, b in zip(g, g_ref))
    assert all(_same_bits(a, b) for a, b in zip(ag[1:], ag_ref[1:]))

    # the attention gradients without the cell's: produced whenever their own pointer is given.  g_cell.weight_ih's pointer
    # is the switch of the cell gradients: without it the other eleven buffers are not written
    g, ag = r.patterns()
    ag = [torch.zeros_like(t) for t in ag]
    assert _same_bits(r.backward([None] + g[1:], ag), dU_ref)
    assert all(_same_bits(a, b) for a, b in zip(ag, ag_ref))
    assert all(_untouched(t) for t in g)
