"""CPU checks of the pieces the training loop's services share (iaf_amd/_capi.py: Handle, destroy, int_in, ptr, StepCounter;
iaf_amd/_recover.py: settle, newly_flagged) on fake objects and a fake library handed in through _capi.lib: no device, no build."""
import ctypes
import gc

import pytest
import torch

from iaf_amd import _capi, _recover


class FakeLib(object):
    """iaf_thing_create / iaf_thing_destroy and the iaf_rng counter calls, each call recorded"""

    def __init__(self, create_status=_capi.IAF_OK):
        self.create_status, self.calls, self.step = create_status, [], 0

    def iaf_error_string(self, code):
        return b"fake"

    def iaf_thing_create(self, out, *args):
        self.calls.append(("create",) + args)
        if self.create_status == _capi.IAF_OK:
            out._obj.value = 0x1000
        return self.create_status

    def iaf_thing_destroy(self, h):
        self.calls.append(("destroy", h))
        return _capi.IAF_OK

    def iaf_rng_seek(self, h, step, st):
        self.step = step
        return _capi.IAF_OK

    def iaf_rng_skip(self, h, steps, st):
        self.step += steps
        return _capi.IAF_OK

    def iaf_rng_tell(self, h, out, st):
        out._obj.value = self.step
        return _capi.IAF_OK

    def iaf_rng_step_ptr(self, h, out):
        out._obj.value = 0x2000
        return _capi.IAF_OK


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_capi, "lib", lambda: lib)
    monkeypatch.setattr(_capi, "_deferred", [])
    monkeypatch.setattr(_capi, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: False)
    return lib


def _destroys(lib):
    return [c for c in lib.calls if c[0] == "destroy"]


def test_handle_destroys_once_with_the_handle_it_exposes(fake):
    own = _capi.Handle("iaf_thing_create", 3, 4)
    h = own.h
    assert isinstance(h, ctypes.c_void_p) and h.value == 0x1000 and fake.calls == [("create", 3, 4)]
    own.close()
    own.close()
    del own
    gc.collect()
    assert len(_destroys(fake)) == 1 and _destroys(fake)[0][1] is h


def test_handle_finaliser_destroys_and_swallows(fake):
    own = _capi.Handle("iaf_thing_create")
    del own
    assert len(_destroys(fake)) == 1
    own = _capi.Handle("iaf_thing_create")
    fake.iaf_thing_destroy = lambda h: 1 / 0
    del own                                   # (an exception in a finaliser must not travel)


def test_handle_never_destroys_what_create_refused(fake):
    fake.create_status = _capi.IAF_ERR_SHAPE
    with pytest.raises(ValueError, match="status -2"):
        _capi.Handle("iaf_thing_create", 1)
    gc.collect()
    assert not _destroys(fake)


def test_destroy_is_put_off_during_a_capture(fake, monkeypatch):
    capturing = [True]
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    a, b = _capi.Handle("iaf_thing_create"), _capi.Handle("iaf_thing_create")
    ha, hb = a.h, b.h
    del a
    assert not _destroys(fake) and [h for _, h in _capi._deferred] == [ha]
    capturing[0] = False
    del b                                     # the next destroy outside a capture makes the call put off, before its own
    assert [c[1] for c in _destroys(fake)] == [ha, hb] and not _capi._deferred


def test_int_in_and_ptr():
    assert _capi.int_in(0, 0, 1) and _capi.int_in(5, 1) and _capi.int_in((1 << 64) - 1, 0, 1 << 64)
    for v in (True, False, 1.0, "1", None, -1, 1 << 64):
        assert not _capi.int_in(v, 0, 1 << 64), v
    assert not _capi.int_in(0, 1) and not _capi.int_in(3, 0, 3)
    t = torch.zeros(4)
    assert _capi.ptr(t).value == t.data_ptr() and not _capi.ptr(None)


def test_step_counter_seek_skip_tell(fake):
    class Source(_capi.StepCounter):
        _prefix = "iaf_rng"
        _h = ctypes.c_void_p(1)
    s = Source()
    s.seek(7)
    s.skip(3)
    s.skip()
    assert s.tell() == 11 and s.counter_ptr() == 0x2000
    for bad in (-1, True, 1.5, 1 << 64):
        with pytest.raises(ValueError, match=r"step must be an int in \[0, 2\*\*64\)"):
            s.seek(bad)
        with pytest.raises(ValueError, match=r"steps must be an int in \[0, 2\*\*64\)"):
            s.skip(bad)
    assert s.tell() == 11


class Obj(object):
    def __init__(self, flag=0):
        self.flag = flag

    def range_errors(self):
        return self.flag


def test_newly_flagged_returns_only_the_unseen_and_grows_seen():
    objs = [Obj(), Obj(1), Obj(), Obj(1)]
    seen = {1}
    assert _recover.newly_flagged(objs, seen) == {3} and seen == {1, 3}
    assert _recover.newly_flagged(objs, seen) == set() and seen == {1, 3}
    objs[0].flag = 2
    assert _recover.flagged(objs) == {0, 1, 3}
    assert _recover.newly_flagged(objs, seen) == {0} and seen == {0, 1, 3}


def _reports(pattern):
    """a compute-only pass that raises a range error where `pattern` says so (and for ever once it runs out, if it ends on one)"""
    calls = []

    def compute():
        calls.append(1)
        if pattern[min(len(calls), len(pattern)) - 1]:
            raise _capi.RangeError("switched")
    return compute, calls


def test_settle_needs_two_clean_passes_in_a_row():
    compute, calls = _reports([1, 0, 1, 0, 0])
    _recover.settle(compute, 3, "Somebody", on_device=False)
    assert len(calls) == 5
    compute, calls = _reports([0, 0])
    _recover.settle(compute, 0, "Somebody", on_device=False)
    assert len(calls) == 2


def test_settle_gives_up_after_its_limit_with_the_callers_name():
    for n in (0, 3):
        compute, calls = _reports([1])
        with pytest.raises(_capi.IafHipError, match="Somebody: objects kept reporting range / exchange failures after %d passes" % (2 * n + 4)):
            _recover.settle(compute, n, "Somebody", on_device=False)
        assert len(calls) == 2 * n + 4
    with pytest.raises(KeyError):             # (another exception is not the protocol's: it travels)
        _recover.settle(lambda: {}["x"], 1, "Somebody", on_device=False)


def test_the_names_read_from_outside_stay():
    from iaf_amd import layers, train
    assert layers._ptr is _capi.ptr and layers._stream is _capi.stream
    assert train._SWITCHED is _recover.SWITCHED and train._range_objects is _recover.range_objects
    assert train._SkipCounter.counter_ptr and _capi.StepCounter.counter_ptr
