"""The pair finder of GanEngine (engine.find_gen_pairs): which discriminator sub-steps can carry the next sub-step's
train-mode generator forward inside their own eval-mode one.  No GPU needed."""
from gan_ffn_amd import engine


def test_reference_schedule_gives_six_pairs_under_every_stream_map():
    assert len(engine.SCHEDULE) == 12
    for n, smap in engine.STREAM_MAP.items():
        pairs = engine.find_gen_pairs(engine.SCHEDULE, smap)
        assert pairs == [0, 2, 4, 6, 8, 10], (n, pairs)
        for i in pairs:
            assert engine.SCHEDULE[i][0] == "D" and engine.SCHEDULE[i + 1][:2] == ("G", engine.SCHEDULE[i][2])


def test_bimodal_schedule_gives_two_pairs():
    assert len(engine.SCHEDULE_BIMODAL) == 4
    for smap in engine.STREAM_MAP_BIMODAL.values():
        assert engine.find_gen_pairs(engine.SCHEDULE_BIMODAL, smap) == [0, 2]


def test_partner_that_is_not_the_next_generator_gives_no_pair():
    sched = [("D", "text", "acoustic"), ("G", "visual", "text"), ("D", "acoustic", "text"), ("D", "visual", "text"),
             ("G", "acoustic", "visual")]
    assert engine.find_gen_pairs(sched, [0] * len(sched)) == []
    # two generator steps in a row, a discriminator step at the end: nothing to pair either
    sched = [("G", "text", "acoustic"), ("G", "acoustic", "text"), ("D", "text", "acoustic")]
    assert engine.find_gen_pairs(sched, [0, 0, 0]) == []


def test_pair_split_over_two_streams_gives_none():
    smap = [0, 1] * 6
    assert engine.find_gen_pairs(engine.SCHEDULE, smap) == []
    smap = [0, 0, 1, 2] + [0] * 8               # only the second pair is split
    assert engine.find_gen_pairs(engine.SCHEDULE, smap) == [0, 4, 6, 8, 10]
