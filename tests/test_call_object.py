"""query._OnStream.call, the one path from Python into the library, without a GPU: a stub scene, a stub library function that
records what it was given, CPU tensors (they have a data_ptr() too) and a stand-in for the device's current stream."""
import types

import pytest
import torch

from ezrt_amd import query, trace

HANDLE, STREAM = 0x5CE2E, 0x57EA4


class _Lib:
    def __init__(self, rc=0):
        self.rc, self.seen = rc, None

    def fn(self, *args):
        self.seen = args
        return self.rc

    def ezrt_last_error(self):
        return b"the stub's last error"


def _on_stream(monkeypatch, lib):
    scene = types.SimpleNamespace(_h=HANDLE, _tl=types.SimpleNamespace(lib=lib))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=STREAM))
    return query._OnStream(scene, torch.device("cpu"), None)


def test_arguments_as_the_library_takes_them(monkeypatch):
    lib = _Lib()
    q = _on_stream(monkeypatch, lib)
    a, b = torch.zeros(5, dtype=torch.float32), torch.zeros((2, 3), dtype=torch.int32)
    q.call(lib.fn, a, None, 7, 0.25, b, True)
    assert lib.seen == (HANDLE, a.data_ptr(), None, 7, 0.25, b.data_ptr(), True, STREAM)
    # tensors as plain ints, ints and floats as they were, the scene handle first and the stream handle last
    assert [type(x) for x in lib.seen] == [int, int, type(None), int, float, int, bool, int]
    assert q.h == STREAM and q.side is False


def test_every_tensor_is_remembered_for_the_closing_step(monkeypatch):
    lib = _Lib()
    q = _on_stream(monkeypatch, lib)
    a, b, c = torch.zeros(1), torch.zeros(2), torch.zeros(3)
    q.call(lib.fn, a, 1, b)
    q.call(lib.fn, None, c, a)
    assert [id(x) for x in q.kept] == [id(a), id(b), id(c), id(a)]
    q.done()                                     # the call's stream is the current one: nothing to record, and the list starts again
    assert q.kept == []


def test_a_nonzero_rc_raises_the_librarys_text(monkeypatch):
    lib = _Lib(rc=-3)
    q = _on_stream(monkeypatch, lib)
    with pytest.raises(trace.TraceError) as e:
        q.call(lib.fn, torch.zeros(1), 4)
    assert str(e.value) == "the stub's last error (rc=-3)"
