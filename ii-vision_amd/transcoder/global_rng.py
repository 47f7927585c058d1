"""Raw access to the two process-wide MT19937 states the reference draws from: `random`'s and `np.random`'s.

Both are 625 words -- 624 of state and a position -- which getstate() / get_state() report and setstate() / set_state() take
at ~15-50 microseconds a call, at every start of a video.Video generator; the 2500 bytes themselves move in under one.  Where
they live is the private business of CPython and numpy, so an address is believed only after the bytes there have been seen
to BE what the public interface reports, before and after a draw that moves the position; otherwise this module goes through
the public interface: slower, same bytes.  The words are always handed over in the public order, state[624] then position."""

import ctypes
import random

import numpy as np


class _GlobalMT:
    """One process-wide MT19937: raw() gives its 625 words as 2500 bytes, write(words) sets them, address() tells where they
    are (0: nowhere that could be verified -- raw / write then use the public interface).  A subclass says what holds the
    state (generator, candidate), how the public interface reads, saves and sets it (words, save, restore, set_words), how to
    move the position (draw), and may override peek / poke / prove / write for what is particular to it."""

    def __init__(self):
        self._gen = self._addr = None     # the generator object the address belongs to, that address or 0

    def peek(self, addr):
        return ctypes.string_at(addr, 2500)

    def poke(self, addr, base):
        ctypes.memmove(addr, base, 2500)

    def prove(self, cand):
        """a further proof of the candidate, made while the caller's state is saved"""
        return True

    def address(self):
        gen = self.generator()
        if self._gen is not gen or gen is None:     # (a generator object that has been replaced is verified anew)
            addr = 0
            try:
                cand = self.candidate(gen)
                if cand:
                    saved = self.save()
                    try:
                        ok = self.peek(cand) == self.words()
                        self.draw()
                        ok = ok and self.peek(cand) == self.words() and self.prove(cand)
                    finally:
                        self.restore(saved)                 # (the caller's stream is where it was)
                    if ok and self.peek(cand) == self.words():
                        addr = cand
            except Exception:
                addr = 0
            self._gen, self._addr = gen, addr
        return self._addr

    def distrust(self, on=True):
        """on: the current generator object's address counts as unverifiable (raw / write go through the public interface)
        until the object is replaced; off: it is verified anew at the next call.  For tests of the fall-back."""
        self._gen, self._addr = (self.generator(), 0) if on else (None, None)

    def raw(self):
        """the 625 words as 2500 bytes: state[624], position"""
        addr = self.address()
        return self.peek(addr) if addr else self.words()

    def write(self, words):
        """the 625 words (a ctypes array / buffer of 2500 bytes, state[624] then position) become the generator's state"""
        addr = self.address()
        if addr:
            self.poke(addr, ctypes.addressof(words) if isinstance(words, ctypes.Array) else np.frombuffer(words, dtype=np.uint8).ctypes.data)
        else:
            self.set_words(np.frombuffer(bytes(words), dtype=np.uint32))


class _PyRandom(_GlobalMT):
    """`random`: CPython _randommodule.c RandomObject -- PyObject_HEAD (of a non-GC base: refcount, type), int index, uint32_t
    state[624] -- while getstate()[1] is state[0..623] followed by index.  The address is derived from the object's own, so it
    is believed only after a write through it has been seen too; a write clears gauss_next, as setstate((3, words, None))
    would."""

    def generator(self):
        return getattr(random, "_inst", None)

    def candidate(self, inst):
        ok = inst is not None and random.getstate.__self__ is inst and type(inst).__mro__[1].__name__ == "Random"
        return id(inst) + object.__basicsize__ if ok else 0

    save = staticmethod(lambda: random.getstate())
    restore = staticmethod(lambda saved: random.setstate(saved))
    draw = staticmethod(lambda: random.getrandbits(8))

    def words(self):
        return np.array(random.getstate()[1], dtype=np.uint32).tobytes()

    def set_words(self, w):
        random.setstate((3, tuple(w.tolist()), None))

    def peek(self, addr):
        return ctypes.string_at(addr + 4, 2496) + ctypes.string_at(addr, 4)

    def poke(self, addr, base):
        ctypes.memmove(addr + 4, base, 2496)
        ctypes.memmove(addr, base + 2496, 4)

    def prove(self, cand):
        probe = np.arange(8, 8 + 625, dtype=np.uint32)
        probe[624] = 3                  # the position
        self.poke(cand, probe.ctypes.data)
        return self.words() == probe.tobytes()

    def write(self, words):
        super().write(words)
        if self._addr:
            self._gen.gauss_next = None


class _NpRandom(_GlobalMT):
    """`np.random`: numpy's mt19937_state (uint32 key[624]; int pos) at BitGenerator.ctypes.state_address, the words
    get_state()[1:3] reports.  A write happens under the bit generator's lock (nobody draws while the words change) and
    leaves has_gauss / cached_gaussian the caller's."""

    def generator(self):
        bg = np.random.mtrand._rand._bit_generator
        if bg is not self._gen and type(bg).__name__ != "MT19937":
            raise RuntimeError("np.random's global generator is not the MT19937 the reference draws from")
        return bg

    def candidate(self, bg):
        return int(bg.ctypes.state_address)

    save = staticmethod(lambda: np.random.get_state())
    restore = staticmethod(lambda saved: np.random.set_state(saved))
    draw = staticmethod(lambda: np.random.random_sample())

    def words(self):
        _, key, pos = np.random.get_state()[:3]
        return np.asarray(key, dtype=np.uint32).tobytes() + np.array([pos], dtype=np.int32).tobytes()

    def set_words(self, w):
        old = np.random.get_state()
        np.random.set_state((old[0], w[:624].copy(), int(w[624]), old[3], old[4]))

    def poke(self, addr, base):
        with self.generator().lock:
            ctypes.memmove(addr, base, 2500)


py_random, np_random = _PyRandom(), _NpRandom()
