#!/usr/bin/env python3
"""Record and compare the C-ABI calls of a test run (the evidence a refactor of the Python layer leaves the device work alone).

    tools/call_trace.py record OUT -- <pytest args>
    tools/call_trace.py diff A B

record wraps every hj_* function of the one `lib` object the package's modules share and runs pytest in this process. OUT
gets one line per test (`# <test id>`) and one per call behind it: the function's name and its arguments -- a scalar as
its value, an argument whose argtypes entry is a pointer as `null` or `ptr`. The package is the first `htm_hashjoin_amd` on
the path, this tree's when there is no other, so another tree's Python files can be recorded over this tree's library.

diff compares two traces test by test. With the memory calls (hj_dev_alloc, hj_dev_free, hj_copy_h2d, hj_copy_d2h) left
out, every difference in the sequence of calls is reported, the first one of a test with both lines. Of the memory calls it
compares, per test, how many there are and how many bytes they copy, and reports what rose from A to B. Exit status 1 when
there is anything to report.
"""
import contextlib
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMORY_CALLS = ("hj_dev_alloc", "hj_dev_free", "hj_copy_h2d", "hj_copy_d2h")
COPIES = ("hj_copy_h2d", "hj_copy_d2h")        # their last argument is the byte count


def _is_pointer(ctype):
    return issubclass(ctype, (C._Pointer, C.c_void_p, C.c_char_p))


def _entry(name, argtypes, args):
    out = [name]
    for ctype, a in zip(argtypes, args):
        value = getattr(a, "value", a)          # a ctypes scalar or pointer object; an array or a byref() has no value
        if _is_pointer(ctype):
            out.append("null" if value is None or (isinstance(value, int) and value == 0) else "ptr")
        else:
            out.append(repr(value.decode() if isinstance(value, bytes) else int(value) if hasattr(value, "__index__") else value))
    return " ".join(out)


@contextlib.contextmanager
def recording(lib, write):
    """every hj_* function of `lib` calls write(entry) before it runs; the functions are put back on leaving"""
    saved = {name: getattr(lib, name) for name in lib._hj_signatures}

    def wrap(name, fn):
        def call(*args):
            write(_entry(name, fn.argtypes, args))
            return fn(*args)
        return call

    for name, fn in saved.items():
        setattr(lib, name, wrap(name, fn))
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


class _TestIds:
    def __init__(self, write):
        self.write = write

    def pytest_runtest_logstart(self, nodeid, location):
        self.write("# " + nodeid)


def record(out_path, pytest_args):
    import pytest
    try:
        import torch  # noqa: F401  (its HIP runtime has to be the first one in the process, as in tests/conftest.py)
    except Exception:  # noqa: BLE001
        pass
    sys.path.append(ROOT)
    import htm_hashjoin_amd as hj
    with open(out_path, "w") as out:
        write = lambda line: out.write(line + "\n")       # noqa: E731
        with recording(hj.lib, write):
            return pytest.main(list(pytest_args), plugins=[_TestIds(write)])


def read_trace(path):
    """{test id: [entries]}, in the order of the file; calls before the first test are under ''"""
    tests = {"": []}
    cur = tests[""]
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("# "):
                cur = tests.setdefault(line[2:], [])
            elif line:
                cur.append(line)
    return tests


def _memory(entries):
    """(number of memory calls, bytes copied)"""
    mem = [e.split() for e in entries if e.split()[0] in MEMORY_CALLS]
    return len(mem), sum(int(e[-1]) for e in mem if e[0] in COPIES)


def diff(a, b):
    """the report lines for two traces as read_trace gives them; empty: nothing differs and nothing rose"""
    report = []
    for test in list(a) + [t for t in b if t not in a]:
        if test not in a or test not in b:
            report.append(f"{test or '(before the first test)'}: only in {'A' if test in a else 'B'}")
            continue
        calls_a, calls_b = ([e for e in t if e.split()[0] not in MEMORY_CALLS] for t in (a[test], b[test]))
        if calls_a != calls_b:
            k = next((i for i, (x, y) in enumerate(zip(calls_a, calls_b)) if x != y), min(len(calls_a), len(calls_b)))
            report.append(f"{test or '(before the first test)'}: call {k} of {len(calls_a)} / {len(calls_b)} differs\n"
                          f"    A: {calls_a[k] if k < len(calls_a) else '(none)'}\n    B: {calls_b[k] if k < len(calls_b) else '(none)'}")
        (n_a, bytes_a), (n_b, bytes_b) = _memory(a[test]), _memory(b[test])
        if n_b > n_a or bytes_b > bytes_a:
            report.append(f"{test or '(before the first test)'}: memory calls {n_a} -> {n_b}, bytes copied {bytes_a} -> {bytes_b}")
    return report


def summary(a, b):
    calls = [sum(len([e for e in t if e.split()[0] not in MEMORY_CALLS]) for t in tr.values()) for tr in (a, b)]
    mem = [[sum(x) for x in zip(*(_memory(t) for t in tr.values()))] for tr in (a, b)]
    return (f"tests {len(a) - 1} / {len(b) - 1}, calls without the memory calls {calls[0]} / {calls[1]}, "
            f"memory calls {mem[0][0]} / {mem[1][0]}, bytes copied {mem[0][1]} / {mem[1][1]}")


def main(argv):
    if len(argv) >= 3 and argv[0] == "record" and argv[2] == "--":
        return int(record(argv[1], argv[3:]))
    if len(argv) == 3 and argv[0] == "diff":
        a, b = read_trace(argv[1]), read_trace(argv[2])
        report = diff(a, b)
        print(summary(a, b))
        print("\n".join(report) if report else "identical without the memory calls; no test's memory calls or copied bytes rose")
        return 1 if report else 0
    sys.exit(__doc__)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
