"""What tests/test_hip_encoder_ranges.py rests on, checked without a GPU (tests/encoder_range_cases.py): every partition tiles
its stack, the deep table stands on both sides of every launch limit, the chunk-count table is what the restated rule gives,
and the fp32 evaluation of the oracle stays inside every bound the GPU module uses — the reference alone passes, and it is
finite and non-trivial down to layer 0 of a 64-layer stack."""
import numpy as np
import pytest
import torch

import encoder_range_cases as RC
from util import _assert_close


def test_every_partition_tiles_its_stack_once_top_down():
    for c, ranges in RC.RANGE_CASES + RC.LEN_CASES:
        assert RC.tiles_top_down(c.L, ranges), (c.L, ranges)
    assert not RC.tiles_top_down(4, ((0, 2), (2, 4)))           # bottom-up
    assert not RC.tiles_top_down(4, ((2, 4), (0, 1)))           # a gap
    assert not RC.tiles_top_down(4, ((2, 4), (1, 3), (0, 1)))   # an overlap
    assert not RC.tiles_top_down(4, ((2, 4), (1, 2)))           # stops above 0
    # the table holds what the issue of this module asks for: both two-way and three-way splits, every layer alone, the
    # engine's buckets; a lower range of one layer, of several; every width at both shapes; a case past 512 tokens
    assert {len(p) for ps in RC.PARTITIONS.values() for p in ps} == {2, 3, 4}
    assert ((5, 8), (2, 5), (0, 2)) in RC.PARTITIONS[8]
    seen = {((c.E, c.H, c.F), (c.S, c.B)) for c, _ in RC.RANGE_CASES if c.train}
    assert all((w, sb) in seen for w in RC.WIDTHS for sb in RC.SHAPES)
    assert any(c.S * c.B >= 512 and (c.E, c.H, c.F) == RC.ROWCHAIN for c, _ in RC.RANGE_CASES)
    assert {(c.E, c.H, c.F) for c, _ in RC.RANGE_CASES if not c.train} == set(RC.WIDTHS)
    for c, _ in RC.LEN_CASES:
        assert 1 in c.lengths and c.S in c.lengths and len(c.lengths) == c.B


def test_deep_table_stands_on_both_sides_of_every_limit():
    rc, gen = RC.DEEP_L[RC.ROWCHAIN], RC.DEEP_L[RC.GENERIC]
    per_launch = RC.GROUP_PROBLEMS // 4                        # layers per grouped weight-gradient launch
    per_reduce = RC.LN_REDUCE_INSTANCES // 2                   # layers per LayerNorm reduce launch
    assert per_launch in rc and per_launch + 1 in rc and per_launch + 1 in gen
    assert per_reduce in rc and per_reduce + 1 in rc and per_reduce + 1 in gen
    assert any(L > 2 * per_launch for L in rc)                 # three launches
    assert RC.MAX_LAYERS in gen
    assert all(c.train and (c.S, c.B) == (5, 2) for c in RC.DEEP_CASES)


def test_chunk_table_is_what_the_rule_gives():
    assert set(RC.SLAB_CHUNKS) == {(L, S * B) for L, S, B in RC.SLAB_CASES}
    for (L, T), n in RC.SLAB_CHUNKS.items():
        assert RC.expected_chunks(L, T)[0] == n, (L, T)
    assert {1, 2}.issubset(RC.SLAB_CHUNKS.values()) and max(RC.SLAB_CHUNKS.values()) >= 3
    # L = 10, T = 1100: the load target's 3 chunks need 3 slabs of the reduce launch, the workspace holds 2 — the clamp binds;
    # the unreduced form's own need (2 gradient-shaped slabs) would fit, and at L = 8 nothing clamps
    assert RC.expected_chunks(10, 1100) == (2, "reduce workspace")
    assert RC.PART_FLOATS // (10 * RC.COVERED_100) == 2 and 1 + RC.PART_FLOATS // (10 * RC.LAYER_FLOATS_100) == 3
    assert RC.expected_chunks(8, 1100) == (3, "target") and RC.expected_chunks(9, 1100) == (2, "reduce workspace")
    assert RC.expected_chunks(8, 3008) == (3, "target")                              # the workload's pass: unchanged
    assert RC.expected_chunks(1, 1100) == (4, "tokens") and RC.expected_chunks(1, 3008) == (8, "cap")


def _reference_alone_passes(c):
    ins = RC.inputs(c)
    per = ins[0].numel()
    r64, r32 = RC.expected(c, ins, RC.seeded_gradients(per))
    n = 0
    for (kind, label, ref), (_, _, got) in zip(RC.quantities(r64, c.L), RC.quantities(r32, c.L)):
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got).all()), label
        e = RC.rel_err(got, ref)
        _assert_close(got.numpy(), ref.numpy(), RC.bound(kind, e), RC.EXISTING[kind][1], label, 0.0, 1.0)
        n += 1
    assert n == 2 + 12 * c.L
    return r64


_SEEN = sorted({RC.case_id(c): c for c, _ in RC.RANGE_CASES + RC.LEN_CASES}.items())


@pytest.mark.parametrize("c", [c for _, c in _SEEN], ids=[i for i, _ in _SEEN])
def test_fp32_oracle_stays_inside_every_range_bound(c):
    _reference_alone_passes(c)


@pytest.mark.parametrize("c", RC.DEEP_CASES, ids=RC.case_id)
def test_fp32_oracle_stays_inside_every_deep_bound(c):
    r64 = _reference_alone_passes(c)
    # the fp64 oracle is finite (checked above) and alive down to layer 0, at L = 64 too: every gradient of layer 0 is
    # within a factor 100 of the same parameter's in the top layer and far above the seeded initial values' 0.05 (see
    # RC.inputs: with the slab as seeded they would be 1e-36 at L = 64)
    g = r64.grads                    # (initial value + gradient: off by at most 0.05)
    top = "transformer_encoder.layers.%d." % (c.L - 1)
    for k in RC.keys(1):
        g0, gt = float(g[k].abs().max()), float(g[top + k.split(".", 3)[3]].abs().max())
        assert g0 > 0.5 and g0 > 0.01 * gt, (k, g0, gt)
    assert float(r64.dx.abs().max()) > 0.1


def test_seeded_gradients_have_no_zero():
    g = RC.seeded_gradients(4096)
    assert bool((g != 0).all()) and float(g.abs().max()) <= 0.05 and float(g.std()) > 0.01
    assert np.array_equal(g.numpy(), RC.seeded_gradients(4096).numpy())
