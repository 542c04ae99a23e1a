"""The class tree of the step runners (engine.py): what every engine shares lives once in _Runner, the network-level operations
once in _NetRunner, and nothing of GanEngine's schedule leaks into the classifier engines.  Needs no GPU."""
import pytest

from gan_ffn_amd import engine

CLASSIFIERS = (engine.Phase2Engine, engine.DrnnEngine, engine.MeldEngine)
GAN_ONLY = ("iteration", "train_disc", "train_gen", "train_gen_forward", "_iteration_body", "loss_dict", "_gen_pair_fwd",
            "_pair_slot", "_use_scratch")


def test_classifier_engines_do_not_derive_from_gan_engine():
    for cls in CLASSIFIERS:
        assert not issubclass(cls, engine.GanEngine), cls
        for name in GAN_ONLY:
            assert not hasattr(cls, name), (cls, name)
    assert issubclass(engine.Phase2Engine, engine._NetRunner) and issubclass(engine.DrnnEngine, engine._NetRunner)
    assert issubclass(engine.GanEngine, engine._NetRunner) and not issubclass(engine.MeldEngine, engine._NetRunner)


def test_shared_methods_exist_once():
    for name in ("_net_fwd", "_net_bwd", "_make_reducer"):
        fn = getattr(engine._NetRunner, name)
        for cls in (engine.GanEngine, engine.Phase2Engine, engine.DrnnEngine):
            assert getattr(cls, name) is fn, (cls, name)
    for name in ("reserve", "_check_slabs"):
        fn = getattr(engine._Runner, name)
        for cls in (engine.GanEngine,) + CLASSIFIERS:
            assert getattr(cls, name) is fn, (cls, name)


def test_runner_has_no_gan_only_class_attribute():
    for name in ("n_streams", "early_gen", "gen_pair", "gen_pair_mode", "_gen_pairs", "_cur_stream", "_base_add", "_adds"):
        assert name not in vars(engine._Runner), name
    assert not hasattr(engine.GanEngine, "early_gen")


class _Stub(engine._Runner):
    """a runner with the capacity state _init_common sets and nothing else"""

    def __init__(self, limit_B=None):
        self._shape = None
        self._cap_S = self._cap_B = self._alloc_S = self._alloc_B = 0
        self.limit_B = limit_B

    def _check_SB(self, S, B):
        if self.limit_B is not None and B > self.limit_B:
            raise ValueError("too many dialogues")


def _state(r):
    return r._shape, (r._cap_S, r._cap_B), (r._alloc_S, r._alloc_B)


def test_capacity_grows_only():
    r = _Stub()
    r.reserve(94, 8)
    assert r._fit(11, 2) == "grow"                       # the first shape allocates at the reserved capacity
    assert _state(r) == ((11, 2), (94, 8), (94, 8))
    assert r._fit(11, 2) == "same" and _state(r) == ((11, 2), (94, 8), (94, 8))
    assert r._fit(5, 1) == "fits"                        # a smaller shape: views only
    assert r._fit(94, 8) == "fits"
    assert _state(r) == ((94, 8), (94, 8), (94, 8))
    assert r._fit(95, 3) == "grow"                       # a longer dialogue: the maximum seen in each dimension
    assert _state(r) == ((95, 3), (95, 8), (95, 8))
    assert r._fit(7, 9) == "grow"                        # a wider batch: S does not shrink
    assert _state(r) == ((7, 9), (95, 9), (95, 9))
    r.reserve(3, 3)                                      # a smaller reservation changes nothing
    assert r._fit(11, 2) == "fits" and _state(r) == ((11, 2), (95, 9), (95, 9))
    r.reserve(110, 4)                                    # a bigger one counts at the next allocation
    assert _state(r) == ((11, 2), (110, 9), (95, 9))
    assert r._fit(96, 2) == "grow" and _state(r) == ((96, 2), (110, 9), (110, 9))


def test_capacity_without_reserve_and_with_a_third_dimension():
    r = _Stub()
    assert r._fit(13, 4, 2, grow=True) == "grow" and _state(r) == ((13, 4, 2), (13, 4), (13, 4))
    assert r._fit(13, 4, 2) == "same"
    assert r._fit(13, 4, 1) == "fits" and r._shape == (13, 4, 1)        # another party count, same (S, B): not "same"
    assert r._fit(11, 2, 3, grow=True) == "grow"         # the caller outgrew its own dimension: allocate, at the same capacity
    assert _state(r) == ((11, 2, 3), (13, 4), (13, 4))


def test_limits_are_checked_by_reserve_and_fit():
    r = _Stub(limit_B=32)
    with pytest.raises(ValueError):
        r.reserve(10, 33)
    with pytest.raises(ValueError):
        r._fit(10, 33)
    assert _state(r) == (None, (0, 0), (0, 0))           # a refused shape leaves no trace
    assert r._fit(10, 32) == "grow"
