"""The library's argument checks, for the CPU tests: option structs built from keywords and the one loop that holds an entry point to
its refusals.  Nothing here launches a kernel: every case fails its check first.  A helper, not a test."""
import ctypes as C
import re

import pytest


def opts(struct, **kw):
    """a zero-initialised `struct` with those of `kw` set that are fields of it"""
    o = struct()
    for k, v in kw.items():
        if hasattr(o, k):
            setattr(o, k, v)
    return o


def assert_refusals(lib, name, make, cases, *extra):
    """Entry point `name`(options, *extra, stream) refuses null options and every (kw, message) of `cases`, options = make(**kw): the
    return value is -1 (PULSE_EINVAL) and the last error is the message under the entry point's name; _native.check raises it (the
    first case).  Returns the errors, one per case."""
    from pulselib_amd import _native
    fn, errors = getattr(lib, name), []
    assert fn(None, *extra, None) == -1 and lib.pulse_last_error() == name.encode() + b": options are null"
    for kw, msg in cases:
        assert fn(C.byref(make(**kw)), *extra, None) == -1, (name, kw)
        errors.append(lib.pulse_last_error())
        assert errors[-1].startswith(name.encode() + b": ") and msg in errors[-1], (name, kw, errors[-1])
    kw, msg = cases[0]
    with pytest.raises(ValueError, match=re.escape(msg.decode())):
        _native.check(fn(C.byref(make(**kw)), *extra, None), name)
    return errors
