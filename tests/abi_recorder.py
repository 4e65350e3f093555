"""A recorder in place of libplonky_hip.so, and the vocabulary the marshalling tests state their expected C calls in
(test_device_marshalling.py, test_api_marshalling.py).  A plain helper module: no fixtures, no pytest settings.

Device pointers are compared with data_ptr(), host limbs by their content read back through the pointer while the wrapper's array
is alive, scalars and sizes by value.  A null pointer counts as one however it is spelt (None or a c_void_p of None).

An entry returns 0 and writes nothing unless the test has queued a reply for it (_Recorder.reply): a status code (or whatever the entry
returns), the text plk_last_error answers with from then on, and values written through byref out-parameters."""
import ctypes
import itertools

import numpy as np
import pytest

NULL = ("ptr", None)
ANYPTR = ("anyptr",)


def P(t):
    """a pointer to this tensor's (or array's) memory"""
    return ("ptr", (t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()) or None)


def H(a, dtype=np.uint64):
    """a pointer to host memory with this content"""
    return ("host", np.ascontiguousarray(a, dtype=dtype).tobytes())


def PA(ts):
    """a ctypes array of pointers"""
    return ("ptrs", [None if t is None else (t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()) for t in ts])


def HA(arrays, dtype=np.uint64):
    """a ctypes array of pointers to host memory with these contents (None: a null entry; nothing to read: any pointer will do)"""
    return ("hosts", [None if a is None else np.ascontiguousarray(a, dtype=dtype).tobytes() for a in arrays])


def VA(values):
    """a ctypes array of these values"""
    return ("ptrs", list(values))


def REF(ctype):
    """byref() of an out-parameter of this type"""
    return ("ref", ctype)


def OUT(i=None):
    """a pointer to what the wrapper returns (its i-th result)"""
    return ("out", i)


def OUTS(i=None):
    """a ctypes array of pointers to the rows of what the wrapper returns (of its i-th result)"""
    return ("outs", i)


def HND(value):
    """a context handle: a c_void_p of this value"""
    return ("hnd", value)


def _snap(arg, want):
    kind = want[0] if isinstance(want, tuple) and want else None
    if kind in ("ptr", "out", "anyptr", "host"):
        if kind == "host" and not want[1] and (arg is None or isinstance(arg, ctypes.c_void_p)):
            return want  # nothing to read: any pointer will do
        if arg is None or (isinstance(arg, ctypes.c_void_p) and arg.value is None):
            return NULL
        if not isinstance(arg, ctypes.c_void_p):
            return ("not a pointer", arg)
        if kind == "host":
            return ("host", ctypes.string_at(arg, len(want[1])))
        return ANYPTR if kind == "anyptr" else ("ptr", arg.value)
    if kind in ("ptrs", "outs"):
        return ("ptrs", list(arg))
    if kind == "hnd":
        return ("hnd", arg.value) if isinstance(arg, ctypes.c_void_p) else ("not a handle", arg)
    if kind == "hosts":
        got = list(arg)
        return ("hosts", [b"" if w == b"" else None if p is None else ctypes.string_at(p, len(w or b"")) for p, w in itertools.zip_longest(got, want[1][:len(got)])])
    if kind == "ref":
        return ("ref", type(arg._obj))
    return arg


class _Recorder:
    def __init__(self):
        self.calls, self.want = [], []
        self.replies, self.last_error = {}, b""

    def reply(self, name, rc=0, error=None, write=None):
        """The next call of entry `name` returns rc, makes plk_last_error answer `error` (where given), and stores write[i] in the
        object behind its i-th argument, a byref out-parameter.  Replies of one entry are used up in the order they were queued."""
        self.replies.setdefault(name, []).append((rc, error, write or {}))

    def __getattr__(self, name):
        if not name.startswith("plk_"):
            raise AttributeError(name)
        if name == "plk_last_error":  # answered, not recorded: how often a wrapper reads the text is its own business
            return lambda: self.last_error

        def entry(*args):
            want = self.want[len(self.calls)][1:] if len(self.calls) < len(self.want) else ()
            self.calls.append((name,) + tuple(_snap(a, w) for a, w in itertools.zip_longest(args, want)))
            if not self.replies.get(name):
                return 0
            rc, error, write = self.replies[name].pop(0)
            for i, value in write.items():
                args[i]._obj.value = value
            if error is not None:
                self.last_error = error.encode() if isinstance(error, str) else error
            return rc

        return entry


def call(rec, want, fn, *args, **kwargs):
    """Run the wrapper, which must make exactly the C call(s) `want`; returns the wrapper's result."""
    wants = want if isinstance(want, list) else [want]
    rec.calls, rec.want = [], wants
    result = fn(*args, **kwargs)

    def resolve(w):
        if isinstance(w, tuple) and w and w[0] == "out":
            r = result if w[1] is None else result[w[1]]
            return NULL if r is None else P(r)
        if isinstance(w, tuple) and w and w[0] == "outs":
            return PA(list(result if w[1] is None else result[w[1]]))
        return w

    assert rec.calls == [tuple(resolve(w) for w in one) for one in wants]
    rec.calls, rec.want = [], []
    return result


def refused(rec, fn, *args, **kwargs):
    rec.calls, rec.want = [], []
    with pytest.raises(AssertionError):
        fn(*args, **kwargs)
    assert rec.calls == []
