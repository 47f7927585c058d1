"""Byte emission of the player opcode stream (.a2m), batched on the GPU, and its inverse: reading a stream back.

Mirrors what movie.Movie.emit_stream / done (transcoder/movie.py:113-161) produce
through opcodes.py / machine.py for one stream, for any number of streams at once
(iiv_emit_stream, csrc/iiv_a2m.hip).  The caller supplies the speaker duty cycle ("tick",
4..66 even, movie.py:104-107) of every opcode: audio.ArrayAudio.ticks() computes them from the
clip's PCM on the device (csrc/iiv_audio.hip), or a constant stands in for a silent movie.

A2mReader takes streams as written -- by emit_stream, by the reference, by an older build -- and checks them (scan), turns them
back into opcodes, ticks and banks (decode) or into the screen memory a player holds after k opcodes (replay), which
native.render_rgb and native.render_error take (iiv_a2m_scan / _decode / _replay, csrc/iiv_a2m_read.hip; include/iivision.h f9).
"""

import numpy as np

import _iiv_native as native
import symbol_table


class OpcodeAddresses:
    """Entry points of the player's opcodes (opcodes.py:168-217)."""

    def __init__(self, tick, ack, terminate, nop=0):
        self.tick = np.ascontiguousarray(tick, dtype=np.uint16).reshape(32, 32)  # [(tick-4)/2][page-32]
        self.ack = int(ack)
        self.terminate = int(terminate)
        self.nop = int(nop)

    @classmethod
    def placeholder(cls):
        """Addresses that give a stream the right layout without a player's debug file: NOT playable, but readable back
        with the same addresses (tools/transcode_clip.py and tools/play_a2m.py without --dbg)."""
        return cls(0x8000 + 16 * np.arange(1024, dtype=np.uint16).reshape(32, 32), 0xc000, 0xc100)

    @classmethod
    def from_debug_file(cls, path="player/iivision.dbg"):
        """Read `op_*` labels from the cc65 debug file, as opcodes._parse_symbol_table does."""
        syms = symbol_table.SymbolTable(path).parse()
        ops = {}
        for name, data in syms.items():
            if name.startswith('"op_'):
                ops[name[4:-1]] = int(data["val"], 16)
        tick = np.zeros((32, 32), dtype=np.uint16)
        for ti, t in enumerate(range(4, 68, 2)):
            for page in range(32, 64):
                key = "tick_%d_page_%d" % (t, page)
                if key not in ops:
                    raise ValueError("Unable to find opcode address for %s in player debug symbols" % key.upper())
                tick[ti, page - 32] = ops[key]
        for key in ("ack", "terminate", "nop"):
            if key not in ops:
                raise ValueError("Unable to find opcode address for %s in player debug symbols" % key.upper())
        return cls(tick, ops["ack"], ops["terminate"], ops["nop"])


def stream_length(mode, n_ops, addresses, max_bytes_out=None):
    return native.emit_stream_size(mode, n_ops, addresses.tick, addresses.ack, addresses.terminate, max_bytes_out)


def emit_stream(mode, ops, ticks, addresses, max_bytes_out=None):
    """ops: CUDA uint8 (n_streams, n_ops, 6) from Encoder.encode / StreamBatch;
    ticks: CUDA uint8 (n_streams, n_ops) -> CUDA uint8 (n_streams, stream_length)."""
    return native.emit_stream(mode, ops, ticks, addresses.tick, addresses.ack, addresses.terminate, max_bytes_out)


class A2mStreamError(ValueError):
    """A stream is not OK: .stream (index in the batch), .status (its name, native.A2M_STATUS), .position (byte)."""

    def __init__(self, stream, status, position):
        super().__init__("stream %d is %s at byte %d" % (stream, status, position))
        self.stream, self.status, self.position = stream, status, position


class A2mReader:
    """Reads .a2m streams on the device with the opcode addresses of one player build."""

    def __init__(self, addresses):
        self.addresses = addresses
        self._reader = native.A2mReaderHandle(addresses.tick, addresses.ack, addresses.terminate)

    def close(self):
        self._reader.close()

    def _batch(self, streams, lengths=None):
        """A list of uint8 arrays / tensors of any lengths, or one 2-D CUDA tensor plus lengths -> (CUDA uint8 (S, stride),
        CUDA int64 (S,)).  Rows are zero behind a stream's own length; the stride is at least 2048."""
        import torch
        if isinstance(streams, torch.Tensor) and streams.dim() == 2:
            if lengths is None:
                raise ValueError("a 2-D tensor of streams needs lengths")
            lengths = torch.as_tensor(np.asarray(lengths, dtype=np.int64) if not isinstance(lengths, torch.Tensor) else lengths)
            return streams.contiguous(), lengths.to(device="cuda", dtype=torch.int64).contiguous()
        rows = [torch.as_tensor(np.frombuffer(r, dtype=np.uint8) if isinstance(r, (bytes, bytearray)) else r).reshape(-1) for r in streams]
        stride = max([2048] + [int(r.numel()) for r in rows])
        data = torch.zeros((len(rows), stride), dtype=torch.uint8, device="cuda")
        for i, r in enumerate(rows):
            if r.dtype != torch.uint8:
                raise ValueError("stream %d is not uint8" % i)
            data[i, :r.numel()] = r.to("cuda")
        return data, torch.tensor([int(r.numel()) for r in rows], dtype=torch.int64, device="cuda")

    def _scanned(self, streams, lengths, strict):
        data, lengths = self._batch(streams, lengths)
        info = self._reader.scan(data, lengths)
        host = info.cpu().numpy()
        if strict:
            for i, (status, _, _, position) in enumerate(host):
                if status != native.A2M_OK:
                    raise A2mStreamError(i, native.A2M_STATUS[int(status)], int(position))
        return data, info, host

    def scan(self, streams, lengths=None):
        """-> int64 numpy (S, 4): {status (native.A2M_STATUS), mode, n_ops, position} of every stream"""
        return self._scanned(streams, lengths, False)[2]

    def decode(self, streams, lengths=None, strict=True):
        """-> [(mode, ops (n_ops, 6), ticks (n_ops,), banks (n_ops,))] per stream, CUDA uint8 views of one batch.
        A stream that is not OK raises A2mStreamError; strict=False decodes its n_ops opcodes anyway."""
        data, info, host = self._scanned(streams, lengths, strict)
        ops, ticks, banks = self._reader.decode(data, info)
        return [(int(host[i, 1]), ops[i, :host[i, 2]], ticks[i, :host[i, 2]], banks[i, :host[i, 2]]) for i in range(len(host))]

    def replay(self, streams, first=0, every=1, n=1, init=None, lengths=None, strict=True):
        """-> (main, aux) CUDA uint8 (S, n, 32, 256): snapshot j is the screen memory after the first
        min(first + j * every, n_ops) opcodes, from init = (main, aux) CUDA uint8 (S, 32, 256) or zeros."""
        data, info, _ = self._scanned(streams, lengths, strict)
        return self._reader.replay(data, info, first, every, n, init)

    def speaker_pcm(self, streams, decim=native.SPEAKER_DECIM, order=native.SPEAKER_ORDER, gain=native.SPEAKER_GAIN, lengths=None,
                    strict=True):
        """-> one CUDA int16 vector per stream: what its ticks sound like on the machine, at audio.speaker_rate(decim) samples a
        second (include/iivision.h f13).  Scan, decode and the speaker kernel follow each other on the device: the kernel takes
        its opcode counts from the scan's own output."""
        data, info, host = self._scanned(streams, lengths, strict)
        _, ticks, _ = self._reader.decode(data, info)
        pcm, _ = native.speaker_pcm(ticks, info[:, 2], decim, order, gain)
        return [pcm[i, :native.speaker_sample_count(int(host[i, 2]), decim)] for i in range(len(host))]


def retarget(stream, old_addresses, new_addresses):
    """One stream written for the player build of old_addresses -> the same movie for new_addresses (CUDA uint8, 1-D):
    decode, then emit_stream.  The banks are a function of the mode and the opcode index, as emit_stream writes them."""
    reader = A2mReader(old_addresses)
    try:
        mode, ops, ticks, _ = reader.decode([stream])[0]
    finally:
        reader.close()
    return emit_stream(mode, ops[None], ticks[None], new_addresses)[0]
