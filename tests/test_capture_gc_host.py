"""The generic path keeps Python's cyclic collector out of its stream captures (pi_mpc._generic._no_collection_while_capturing):
dead reference cycles that own device objects are collected BEFORE the capture, nothing is collected inside it, and the
collector is back on afterwards — also when the capture raises, and left off for a caller who had switched it off."""
import gc

import pytest

from pi_mpc._generic import _no_collection_while_capturing


class _Cycle:
    finalised = []

    def __init__(self, name):
        self.me, self.name = self, name

    def __del__(self):
        _Cycle.finalised.append(self.name)


def test_collects_before_and_not_inside():
    assert gc.isenabled()
    _Cycle.finalised.clear()
    _Cycle("before")
    with _no_collection_while_capturing():
        assert _Cycle.finalised == ["before"] and not gc.isenabled()
        _Cycle("inside")
        junk = [[] for _ in range(5000)]  # (far past the young generation's threshold: an enabled collector would have run)
        del junk
        assert _Cycle.finalised == ["before"]
    assert gc.isenabled()
    gc.collect()
    assert _Cycle.finalised == ["before", "inside"]


def test_collector_comes_back_after_an_error_and_stays_off_for_a_caller_who_disabled_it():
    with pytest.raises(RuntimeError):
        with _no_collection_while_capturing():
            raise RuntimeError("capture failed")
    assert gc.isenabled()
    gc.disable()
    try:
        with _no_collection_while_capturing():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
