"""The stream-order probe: one call of the C ABI made on a busy, non-blocking side stream, arranged so that work issued on any
other stream than the one the caller named, or a host array read after the call returned, changes the bytes that come out.

Every GPU test that runs on torch's default stream runs on the legacy null stream, which orders itself against everything: a
kernel, memset or copy issued on stream 0 instead of `stream` gives the right bytes there.  The protocol:

  before anything is enqueued   the device inputs hold a DECOY (valid content, another result), the outputs sentinel A, and a
                                warm-up call of the same shape has run and been synchronised (the caller's job)
  on `side`, in this order      _sleep(SLEEP_CYCLES); the real inputs are copied over the decoys; the outputs are filled with
                                sentinel B; the call under test; the decoys are copied back over the inputs
  right after the call returns  every host array the header says is read before return is overwritten with valid, different values
  busy = not side.query()       taken after the last enqueue: an asynchronous entry point must leave the stream busy -- which is
                                also what makes the probe valid (a drained stream proves nothing): a false `busy` FAILS
  side.synchronize()            and the caller compares the outputs with the model of the REAL inputs; bytes the call does not
                                own must still hold sentinel B

The side stream must be one that the null stream really runs beside.  HIP spreads its streams over a few hardware queues
(GPU_MAX_HW_QUEUES, 4 by default), and a stream that shares its queue with the null stream has the null stream's work executed
in submission order BEHIND its own sleep -- the right order, by accident: such a probe is blind.  independent_stream() therefore
takes fresh streams until it has one on which a sleeping kernel demonstrably does not hold back a null-stream operation (each
pool stream is tried once per process), and every probe shows the same again under its own sleep: a marker enqueued on the
null stream right behind the sleep must finish while the side stream is still asleep, or the probe FAILS.

Work issued on the null stream runs during the sleep: it reads the decoy, or sentinel B overwrites what it wrote.  A zeroing
memset issued early is overwritten by sentinel B.  Work deferred to another stream reads the restored decoy.  A host array
read late sees the scribble.  Nothing here is ever out of range: a library that is wrong computes wrong bytes, it does not fault.
"""
import numpy as np

SLEEP_CYCLES = 200_000_000   # torch.cuda._sleep argument in front of every probe: what tests/test_gpu_resize.py uses
SENTINEL_A, SENTINEL_B = 0xA5, 0x5B


CHECK_CYCLES = SLEEP_CYCLES // 8   # the sleep independent_stream() tries a stream with
_runs_beside_null = {}            # hipStream_t -> does the null stream run beside it (per process)


def _null_overtakes(side, marker):
    """With `side` busy: does an operation enqueued on the null stream now finish before `side` drains?"""
    import torch
    null = torch.cuda.default_stream()
    with torch.cuda.stream(null):
        marker.add_(1)
    while not side.query():
        if null.query():
            return True
    return False


def independent_stream():
    """A fresh torch stream (non-blocking: the null stream does not wait for it) that does not share the null stream's place in
    a hardware queue; AssertionError if 64 fresh streams give none."""
    import torch
    marker = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(64):
        side = torch.cuda.Stream()
        key = side.cuda_stream
        if key not in _runs_beside_null:
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                torch.cuda._sleep(CHECK_CYCLES)
            _runs_beside_null[key] = _null_overtakes(side, marker)
            side.synchronize()
        if _runs_beside_null[key]:
            return side
    raise AssertionError("no stream found that the null stream runs beside: %r" % (sorted(_runs_beside_null.values()),))


class Probe:
    """One probe.  Build it (input / output / host), hand run() the call, then compare."""

    def __init__(self):
        import torch
        self.torch = torch
        self.side = independent_stream()
        self._marker = torch.zeros(1, dtype=torch.int32, device="cuda")
        self._inputs, self._outputs, self._host, self._scribbles = [], [], [], []
        self.busy = None

    def input(self, real, decoy):
        """A device input: holds `decoy` now, `real` only while the call under test runs.  numpy arrays of one shape and dtype."""
        real, decoy = np.ascontiguousarray(real), np.ascontiguousarray(decoy)
        assert real.shape == decoy.shape and real.dtype == decoy.dtype and not np.array_equal(real, decoy)
        t = self.torch
        live = t.from_numpy(decoy.copy()).cuda()
        self._inputs.append((live, t.from_numpy(real.copy()).cuda(), t.from_numpy(decoy.copy()).cuda(), None))
        return live

    def in_place(self, real, decoy):
        """A device buffer the call reads AND rewrites (device tensors, not the same content): -> (live, kept); `kept` receives
        what the call left in `live`, copied on the side stream before the decoy goes back over it."""
        t = self.torch
        assert real.shape == decoy.shape and real.dtype == decoy.dtype and real.is_contiguous() and decoy.is_contiguous()
        live, kept = decoy.clone(), t.empty_like(decoy)
        self.bytes_of(kept).fill_(SENTINEL_A)
        self._inputs.append((live, real, decoy, kept))
        return live, kept

    def output(self, shape, dtype=None):
        """A device output, every byte sentinel A (sentinel B once the probe runs)."""
        t = self.torch
        out = t.empty(shape, dtype=dtype or t.uint8, device="cuda")
        self.bytes_of(out).fill_(SENTINEL_A)
        self._outputs.append(out)
        return out

    def host(self, real, scribble):
        """A host array the call reads before it returns: the array to pass (owned here), overwritten with `scribble` right
        after the call."""
        a = np.ascontiguousarray(real).copy()
        s = np.ascontiguousarray(scribble, dtype=a.dtype).reshape(a.shape)
        assert not np.array_equal(a, s)
        self._host.append((a, s))
        return a

    def scribble(self, fn):
        """fn() overwrites a host array that is no numpy array (a ctypes array of segments); run right after the call"""
        self._scribbles.append(fn)

    @staticmethod
    def bytes_of(tensor):
        import torch
        return tensor.view(-1).view(torch.uint8)

    @staticmethod
    def sentinel(shape, dtype=np.uint8):
        """what an untouched output holds after the probe, as a numpy array"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.full(n, SENTINEL_B, np.uint8).view(dtype).reshape(shape)

    def begin(self, null_sleep=0, synchronize=True):
        """The probe up to the call under test, enqueued on the side stream: the sleep, the marker, the real inputs, sentinel B.
        null_sleep: cycles of a second sleep put on the NULL stream behind the marker (tests/test_gpu_cold_paths.py: what a
        first use issues on the null stream then runs late instead of early).  synchronize=False: another probe is already
        asleep on its own stream (two encoders side by side)."""
        t = self.torch
        if synchronize:
            t.cuda.synchronize()
        with t.cuda.stream(self.side):
            t.cuda._sleep(SLEEP_CYCLES)
            # the null stream runs beside this stream NOW, under this probe's own sleep: what the call issues on it runs ahead
            self.beside = _null_overtakes(self.side, self._marker)
            if null_sleep:
                with t.cuda.stream(t.cuda.default_stream()):
                    t.cuda._sleep(null_sleep)
            for live, real, _, _ in self._inputs:
                live.copy_(real, non_blocking=True)
            for out in self._outputs:
                self.bytes_of(out).fill_(SENTINEL_B)

    def end(self, asynchronous=True):
        """Right after the call(s) returned: the scribbles, the decoys back, `busy`, the synchronise and the probe's own conditions."""
        t = self.torch
        with t.cuda.stream(self.side):
            for a, s in self._host:
                a[...] = s
            for fn in self._scribbles:
                fn()
            for live, _, decoy, kept in self._inputs:
                if kept is not None:
                    kept.copy_(live, non_blocking=True)
                live.copy_(decoy, non_blocking=True)
            self.busy = not self.side.query()
        self.side.synchronize()
        assert self.beside, "a null-stream operation did not run ahead of the sleeping side stream: the probe would be blind"
        if asynchronous:
            assert self.busy, "the side stream had drained when the call returned: the call synchronised, or the sleep is too short"

    def run(self, call, asynchronous=True, null_sleep=0):
        """call(stream_pointer) makes the call(s) under test and returns what the caller wants back.
        asynchronous=False: a synchronising entry point -- same protocol, no `busy` condition."""
        import ctypes
        self.begin(null_sleep)
        with self.torch.cuda.stream(self.side):
            result = call(ctypes.c_void_p(self.side.cuda_stream))
        self.end(asynchronous)
        return result
