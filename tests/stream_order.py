"""What the stream-order tests share (test_gpu_stream_order.py, test_stream_contract.py): a bounded delay on a torch stream,
device buffers staged so that a call which reads or writes out of stream order computes a WRONG answer and never an invalid
one, the driver of one delayed sequence, the witness that the delay and the decoys mean something, and the parser of the
"Stream contract" table of INTEGRATION.md. No test in here, and nothing that asks the library what a result should be.

The discipline. Every device buffer is a torch tensor that exists before the delay; the library gets its data_ptr(). Before
the delay, synchronously, every input holds a DECOY -- valid content that gives a different, known result (an R disjoint
from S, HJ_NO_ROW maps, agg_common.POISON values, all-zero validity planes, all-zero offsets) -- and every output the
sentinel, with guard bytes in front of and behind every buffer. Behind the delay, on the same stream, the real inputs arrive
from pinned host memory, then the library's calls are enqueued, then a torch copy on the same stream takes the outputs to
pinned host memory. A call that went to another stream, or a host read that should have waited, sees the decoy. No decoy is
out of range as a key, a row or an offset."""
import os
import re
import time

import numpy as np

try:
    import torch
except Exception:  # noqa: BLE001  (the contract parser below needs no torch)
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The one delay every sequence waits behind, in milliseconds. Measured on an MI355X (profiles/stream_order.md): the longest
# host-side enqueue of a sequence, two contexts interleaved, took 1.16 ms; 20 x that is 23 ms, below the floor of 50 ms. 100 ms
# is 86 x the longest enqueue -- the host time varies with the load of a shared machine -- and keeps the whole file at about
# five seconds. A delay that is too short shows up as a failed pending() assertion, never as a silent pass.
DELAY_MS = 100.0

GUARD_BYTES = 4096               # in front of and behind every staged buffer: a multiple of every alignment the library asks for
SENT_BYTE = 0xA5
SENT32 = 0xA5A5A5A5
SENT64 = 0xA5A5A5A5A5A5A5A5
NO_ROW = 0xFFFFFFFF

ENQUEUE_MS = {}                  # tag -> host milliseconds of the last delayed enqueue (what profiles/stream_order.md quotes)
CALIBRATION = {}                 # "cycles_per_ms" (or "matmuls_per_ms"), "probe_cycles", "probe_ms": the calibration seen


# ---- the delay ----------------------------------------------------------------------------------------------------------
def _timed_ms(stream, work):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        work()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


_SPIN = {}


def _matmul_chain(k):
    m = _SPIN.setdefault("m", torch.ones((2048, 2048), device="cuda", dtype=torch.float32))
    out = _SPIN.setdefault("out", torch.empty_like(m))
    for _ in range(k):
        torch.mm(m, m, out=out)


def calibrate():
    """cycles of torch.cuda._sleep per millisecond (a chain of large matmuls where this torch has no _sleep), timed once with
    torch events on a side stream: the probe grows until it takes at least 2 ms, so that launch latency is noise"""
    if CALIBRATION:
        return CALIBRATION
    stream = torch.cuda.Stream()
    if hasattr(torch.cuda, "_sleep"):
        unit, work, n = "cycles_per_ms", (lambda c: torch.cuda._sleep(int(c))), 1_000_000
    else:
        unit, work, n = "matmuls_per_ms", _matmul_chain, 4
    _timed_ms(stream, lambda: work(n))                      # first launch: code object load
    for _ in range(8):
        ms = _timed_ms(stream, lambda: work(n))
        if ms >= 2.0:
            break
        n *= 4
    CALIBRATION.update({"unit": unit, unit: n / ms, "probe": n, "probe_ms": ms})
    print("stream_order calibration:", CALIBRATION)
    return CALIBRATION


class Delayed:
    """A bounded delay of `ms` milliseconds enqueued on `stream`, and an event behind it. Always finite: nothing waits on a
    host flag."""

    def __init__(self, stream, ms=None):
        cal = calibrate()
        self.ms = DELAY_MS if ms is None else ms
        amount = max(1, int(self.ms * cal[cal["unit"]]))
        with torch.cuda.stream(stream):
            if cal["unit"] == "cycles_per_ms":
                torch.cuda._sleep(amount)
            else:
                _matmul_chain(amount)
            self.after_delay = torch.cuda.Event()
            self.after_delay.record(stream)

    def pending(self):
        return not self.after_delay.query()


# ---- stream flavours ------------------------------------------------------------------------------------------------------
class Flavour:
    """a stream as torch sees it and as the library takes it (hj_create_on_stream). "side": a torch.cuda.Stream(), which is
    non-blocking; "null": handle 0, the legacy default stream that torch.cuda.current_stream() is unless something changed it"""

    def __init__(self, name):
        self.name = name
        self.stream = torch.cuda.Stream() if name == "side" else torch.cuda.default_stream()
        self.handle = self.stream.cuda_stream
        assert (self.handle == 0) == (name == "null"), (name, self.handle)


FLAVOURS = ("side", "null")


# ---- staged buffers -------------------------------------------------------------------------------------------------------
def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Buf:
    """one staged device buffer: GUARD_BYTES of sentinel, the body, GUARD_BYTES of sentinel. ptr is the body's address"""

    def __init__(self, decoy, inputs, fetch):
        body = _bytes(decoy)
        self.n = body.size
        image = np.full(self.n + 2 * GUARD_BYTES, SENT_BYTE, dtype=np.uint8)
        image[GUARD_BYTES:GUARD_BYTES + self.n] = body
        self.image = torch.from_numpy(image).pin_memory()
        self.dev = torch.empty(image.size, dtype=torch.uint8, device="cuda")
        self.ptr = self.dev.data_ptr() + GUARD_BYTES
        assert self.ptr % 16 == 0
        self.inputs = {}
        for which, a in inputs.items():
            a = _bytes(a)
            assert a.size == self.n, (which, a.size, self.n)
            self.inputs[which] = torch.from_numpy(a.copy()).pin_memory()
        self.back = torch.empty(image.size, dtype=torch.uint8).pin_memory() if fetch else None

    def body(self):
        return self.dev[GUARD_BYTES:GUARD_BYTES + self.n]


class Stage:
    """the staged buffers of one context's sequence on one stream"""

    def __init__(self, stream):
        self.stream, self.bufs = stream, []

    def buf(self, decoy, real=None, warm=None, fetch=False):
        """decoy: what the body holds before the delay (an input's decoy, an output's sentinel or prefill). real / warm: an
        input's content behind the delay, and in the warm-up: other valid content of the same size. fetch: the consumer
        copies the buffer back"""
        assert (real is None) == (warm is None)
        b = Buf(decoy, {} if real is None else {"real": real, "warm": warm}, fetch)
        self.bufs.append(b)
        return b

    def out(self, n, dtype, fill):
        """an output of n elements prefilled with `fill`, fetched"""
        return self.buf(np.full(n, fill, dtype=dtype), fetch=True)

    def arm(self):
        """decoys and sentinels everywhere, synchronously"""
        with torch.cuda.stream(self.stream):
            for b in self.bufs:
                b.dev.copy_(b.image, non_blocking=True)
        self.stream.synchronize()

    def load(self, which):
        with torch.cuda.stream(self.stream):
            for b in self.bufs:
                if b.inputs:
                    b.body().copy_(b.inputs[which], non_blocking=True)

    def download(self, stream=None):
        """the consumer: every fetched buffer to pinned host memory, on the stage's stream (`stream`: the witness's misuse)"""
        stream = self.stream if stream is None else stream
        with torch.cuda.stream(stream):
            for b in self.bufs:
                if b.back is not None:
                    b.back.copy_(b.dev, non_blocking=True)

    def result(self, b, dtype, tag=None):
        """the body of a fetched buffer as the consumer saw it, its guard bytes checked"""
        a = b.back.numpy()
        assert (a[:GUARD_BYTES] == SENT_BYTE).all(), (tag, "a byte in front of the buffer was written")
        assert (a[GUARD_BYTES + b.n:] == SENT_BYTE).all(), (tag, "a byte behind the buffer was written")
        return a[GUARD_BYTES:GUARD_BYTES + b.n].view(dtype).copy()

    def check_inputs_intact(self, tag=None):
        """(after the final sync) no call wrote into the guards of an input either"""
        for b in self.bufs:
            if b.back is None:
                a = b.dev.cpu().numpy()
                assert (a[:GUARD_BYTES] == SENT_BYTE).all() and (a[GUARD_BYTES + b.n:] == SENT_BYTE).all(), (tag, "guard of an input")


def _streams(stages):
    out = []
    for st in stages:
        if all(st.stream is not s for s in out):
            out.append(st.stream)
    return out


def run_delayed(stages, seq, asynchronous, tag, before_real=None):
    """One sequence. seq(which) enqueues the library's calls for the inputs `which` ("warm", then "real"); the host counts a
    call needs come from the test's numpy reference for that input set. The warm-up (other valid inputs of the same sizes,
    so that every buffer of the library has grown) is followed by a sync; then decoys and sentinels again, ONE delay per
    stream, the real inputs, the calls, the consumer -- no host sync in between -- and one final synchronize per stream.
    asynchronous: assert that the delay was still pending after the last enqueue, i.e. that no call blocked the host and that
    every call was enqueued while its inputs still held the decoys. -> host milliseconds of the delayed enqueue"""
    streams = _streams(stages)
    try:
        for st in stages:
            st.arm()
        for st in stages:
            st.load("warm")
        seq("warm")
        for s in streams:
            s.synchronize()
        for st in stages:
            st.arm()
        if before_real is not None:
            before_real()
        delays = [Delayed(s) for s in streams]
        t0 = time.perf_counter()
        for st in stages:
            st.load("real")
        seq("real")
        for st in stages:
            st.download()
        ms = (time.perf_counter() - t0) * 1e3
        still = [d.pending() for d in delays]
    finally:
        for s in streams:
            s.synchronize()
    ENQUEUE_MS[tag] = ms
    print(f"stream_order enqueue {tag}: {ms:.3f} ms host, delay {DELAY_MS:.0f} ms, pending after enqueue {still}")
    if asynchronous:
        assert all(still), (tag, f"the delay of {DELAY_MS} ms had run out after an enqueue of {ms:.3f} ms: a call blocked the host, "
                                 "or the delay is too short for this host")
    return ms


# ---- the witness ----------------------------------------------------------------------------------------------------------
def witness(flavour):
    """The harness misused on purpose: the consumer copy goes to ANOTHER stream than the delayed one. It must return the
    decoy, while the delay is still pending -- the proof that the delay outlasts an enqueue and that a mis-ordered read is
    visible. Without it every stream-order test could pass vacuously."""
    real = np.arange(1, 1 + (1 << 16), dtype=np.uint64)
    decoy = real + np.uint64(1 << 20)
    st = Stage(flavour.stream)
    b = st.buf(decoy, real=real, warm=real, fetch=True)
    other = torch.cuda.Stream()
    st.arm()
    try:
        d = Delayed(flavour.stream)
        st.load("real")
        st.download(stream=other)
        other.synchronize()
        still = d.pending()
        early = st.result(b, np.uint64, "witness")
    finally:
        flavour.stream.synchronize()
    st.download()
    flavour.stream.synchronize()
    late = st.result(b, np.uint64, "witness")
    assert still, "the delay had run out before a copy on another stream finished: the delay is too short to order anything"
    assert np.array_equal(early, decoy) and not np.array_equal(decoy, real), "a consumer on another stream did not see the decoy"
    assert np.array_equal(late, real), "a consumer on the delayed stream did not see the real input"
    return True


# ---- the contract table of INTEGRATION.md ---------------------------------------------------------------------------------
CLASSES = ("asynchronous", "reads back", "waits", "no device work")


def contract(path=None):
    """{entry point: (class, note)} from the table under the heading "Stream contract" of INTEGRATION.md; a name that appears
    twice, a row without a name or a table that is missing raises"""
    text = open(path or os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^#+ .*Stream contract.*$", text, re.M)
    if not m:
        raise ValueError("INTEGRATION.md has no 'Stream contract' section")
    rows, started = {}, False
    for line in text[m.end():].splitlines():
        if not line.startswith("|"):
            if started:
                break                                       # the table is one block of lines
            continue
        started = True
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) < 2 or set(cells[0]) <= set("-: ") or cells[0].lower() == "entry point":
            continue                                        # the header row and the rule under it
        names = re.findall(r"`(hj_[a-z0-9_]+)`", cells[0])
        if len(names) != 1:
            raise ValueError(f"stream contract: one entry point per row, not {cells[0]!r}")
        if names[0] in rows:
            raise ValueError(f"stream contract: {names[0]} appears twice")
        rows[names[0]] = (cells[1], cells[2] if len(cells) > 2 else "")
    if not rows:
        raise ValueError("the 'Stream contract' section holds no table")
    return rows


def asynchronous_calls():
    """the entry points the table classifies as asynchronous in the steady state: where a delayed sequence is made of these
    alone, the delay must still be pending after the last enqueue"""
    return {name for name, (cls, _note) in contract().items() if cls == "asynchronous"}
