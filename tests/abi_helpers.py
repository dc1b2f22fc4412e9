"""Shared pieces of the tests/test_*_abi.py files (CPU): the symbol check, host stand-ins for device pointers and the
refusal loop.  The CASES / ROWS / LIGHT / MESSAGE tables, and the argument order of each entry point, stay in the files."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_symbols(fns, python_names=(), version=4):
    """every name of `fns` is declared in include/hf.h (both kinds of comment stripped), exported by libhf.so and bound
    by _capi; HF_VERSION is `version` (a feature is detected by its symbols); every name of `python_names` is a
    callable of the package.  Returns the stripped header for a file that looks for more in it."""
    import hf_amd
    from hf_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "hf.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    lib = C.CDLL(hf_amd.build.LIB_PATH)
    for fn in fns:
        assert re.search(rf"\b{fn}\s*\(", hdr), f"{fn} not declared in include/hf.h"
        assert hasattr(lib, fn), fn
        assert fn in _capi.SYMBOLS, fn
    assert _capi.lib().hf_version() == version
    for name in python_names:
        assert callable(getattr(hf_amd, name)), name
    return hdr


def stand_ins(null=(), null_row=None):
    """(rows, arg): host addresses that stand in for device pointers (and for the handle: no case gets as far as reading
    one).  arg(name) is the address of one buffer of 16384 floats, or None if `name` is in `null`; rows(name, k) is an
    array of k such addresses, None if `name` is in `null`, with its last entry None if `name` is `null_row`.  The
    buffer lives as long as either closure does."""
    from hf_amd import _capi
    keep = (C.c_float * 16384)()

    def arg(name, offset=0):
        return None if name in null else C.addressof(keep) + offset

    def rows(name, k=3):
        if name in null:
            return None
        r = (_capi._fp * k)(*([C.addressof(keep)] * k))
        if null_row == name:
            r[k - 1] = None
        return r
    return rows, arg


def assert_refused(call, fn, cases, message=None):
    """call(lib, fn, **kw) returns HF_EINVAL for every kw of `cases` and leaves a message that starts with "fn:"; with
    `message`, the message also holds the fragment filed under the case's first key ("spp" wherever it is one)"""
    from hf_amd import _capi
    lib = _capi.lib()
    for kw in cases:
        assert call(lib, fn, **kw) == _capi.HF_EINVAL, kw
        msg = lib.hf_last_error_string().decode()
        assert msg.startswith(fn + ":"), (kw, msg)
        if message is not None:
            first = "spp" if "spp" in kw else next(iter(kw))
            assert message[first] in msg, (kw, msg)
