"""The library's argument checks, for the CPU tests: option structs built from keywords and the one loop that holds an entry point to
its refusals.  Nothing here launches a kernel: every case fails its check first.  And the compiler's resource remarks of a unit's
kernels.  A helper, not a test."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "pulselib_amd" / "csrc"
_WORDS = (C.c_int64 * 8)()
PTR = C.addressof(_WORDS)                  # host words for a struct's buffers: they pass every null and alignment check, and no refusal reads them
assert PTR % 16 == 0


def opts(struct, **kw):
    """a zero-initialised `struct` with those of `kw` set that are fields of it"""
    o = struct()
    for k, v in kw.items():
        if hasattr(o, k):
            setattr(o, k, v)
    return o


def nt_opts(struct, defaults, **kw):
    """A zero-initialised struct of the n-tuple network's entry points with `defaults`, then `kw` over them.  `tuples` = a list of cell
    lists; net_* go to the network, where net_n_tuples and net_n_weights default to what `tuples` says and net_lenK replaces tuple K's
    length; every other keyword is a field of the struct (KeyError otherwise)."""
    o, base = struct(), {**defaults, **kw}
    fields = {f[0] for f in struct._fields_}
    tuples = base.pop("tuples")
    o.net.n_tuples = base.pop("net_n_tuples", len(tuples))
    for t, cells in enumerate(tuples[:8]):
        o.net.tuple_len[t] = base.pop("net_len%d" % t, len(cells))
        for i, c in enumerate(cells):
            o.net.cells[t][i] = c
    o.net.n_weights = base.pop("net_n_weights", sum(16 ** len(c) for c in tuples))
    for k, v in base.items():
        if k.startswith("net_"):
            setattr(o.net, k[4:], v)
        elif k in fields:
            setattr(o, k, v)
        else:
            raise KeyError(k)
    return o


@functools.lru_cache(maxsize=None)
def remarks(target):
    """the compiler's resource remarks of `make <target>` in csrc (one of its *-resource-usage targets), as it printed them; one
    compiler run per target and session"""
    run = subprocess.run(["make", "-s", "-C", str(CSRC), target], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stderr


def resource_usage(target):
    """(names, vgprs, scratch, spills), one entry per kernel of remarks(target), printed as name -> VGPRs"""
    text = remarks(target)
    names = re.findall(r"Function Name: (\S+)", text)
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", text)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", text)]
    print(dict(zip(names, vgprs)))
    return names, vgprs, scratch, spills


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
