"""Encodes an input audio stream into a sequence of speaker duty cycle counts (transcoder/audio.py), on the GPU.

The reference decodes with audioread and resamples each decode block with librosa / scipy on the host; here the PCM is
handed to the device and csrc/iiv_audio.hip does the channel mean, the resample, the normalisation and the quantisation
(include/iivision.h: iiv_audio_*).  `Audio` keeps the reference's interface, so that its movie.py runs with this module in
place of its own; `ArrayAudio` is the array form, batched over streams, like
frame_grabber.ArrayFrameGrabber.

Decoding: 16-bit PCM .wav files are read with the standard library's `wave` module.  audioread's other backends (ffmpeg,
GStreamer, Core Audio, MAD) are not part of this package; any other file fails with a message that says so.
"""
import wave
from typing import Iterator

import numpy as np

import _iiv_native as native

BITRATE = native.AUDIO_BITRATE
BLOCK_FRAMES = native.AUDIO_BLOCK_FRAMES
CLOCK = 1020484   # cycles a second of the Apple II the player runs on (NTSC: 14.31818 MHz * 65 / 912)


def speaker_rate(decim=native.SPEAKER_DECIM, clock=CLOCK):
    """Samples a second of speaker_pcm at one sample per `decim` cycles: the one place where the machine's clock enters (the
    kernel counts cycles only).  decim = 23 gives 44 369 Hz."""
    return int(round(clock / decim))


def read_wav(filename):
    """16-bit PCM .wav -> (int16 (n_frames, channels), sample rate)"""
    try:
        w = wave.open(filename, "rb")
    except (wave.Error, EOFError) as e:
        raise ValueError("%s: not a PCM .wav file (%s); only 16-bit PCM .wav is decoded here -- the reference's other "
                         "decoders (audioread: ffmpeg, GStreamer, Core Audio, MAD) are not available" % (filename, e))
    with w:
        if w.getsampwidth() != 2:
            raise ValueError("%s: %d-bit samples; only 16-bit PCM .wav is decoded here (no audioread decoder)" % (
                filename, 8 * w.getsampwidth()))
        ch, rate, n = w.getnchannels(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    pcm = np.frombuffer(raw, dtype="<i2").astype(np.int16).reshape(-1, ch)
    return pcm, rate


def write_wav(filename, pcm, rate):
    """int16 (n,) -> a 16-bit mono PCM .wav at `rate` Hz"""
    with wave.open(filename, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


class ArrayAudio:
    """PCM already in memory: int16 (n_frames, channels) or (n_frames,) for one stream, or (n_streams, n_frames,
    channels) for a batch of equally long streams (numpy or torch; a CUDA tensor is used in place).  normalization: one
    value or one per stream; None = Audio._normalization of each stream, on the device.  block_frames: frames per decode
    block (audio.py:98 reads 128 * 1024)."""

    def __init__(self, pcm, rate, bitrate: int = BITRATE, normalization=None, block_frames: int = BLOCK_FRAMES):
        torch = native._torch()   # (no GPU: RuntimeError, there is no CPU fallback)
        t = pcm if isinstance(pcm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16))
        if t.dtype != torch.int16:
            raise ValueError("pcm must be int16")
        if t.dim() == 1:
            t = t[:, None]
        if t.dim() == 2:
            t = t[None]
        if t.dim() != 3:
            raise ValueError("pcm: (n_frames,), (n_frames, channels) or (n_streams, n_frames, channels)")
        self.n_streams, self.n_frames, self.channels = (int(x) for x in t.shape)
        self.pcm = t.reshape(self.n_streams, self.n_frames * self.channels).to("cuda").contiguous()
        self.rate = int(rate)
        self.bitrate = int(bitrate)
        self.sample_rate = float(bitrate)
        self.block_frames = int(block_frames)
        if normalization is None:
            normalization = native.audio_normalization(self.pcm, self.n_frames, self.channels, self.rate, self.bitrate)
        self.normalization = np.broadcast_to(np.asarray(normalization, dtype=np.float64), (self.n_streams,)).copy()

    def tick_count(self):
        return native.audio_tick_count(self.n_frames, self.rate, self.bitrate, self.block_frames)

    def ticks(self, out=None):
        """CUDA uint8 (n_streams, tick_count()): the speaker duty cycle (4..66, even) of every opcode of every stream.
        Asynchronous on torch's current stream."""
        t, _ = native.audio_ticks(self.pcm, self.n_frames, self.channels, self.rate, self.normalization, self.bitrate,
                                  self.block_frames, out)
        return t

    def speaker_pcm(self, decim=native.SPEAKER_DECIM, order=native.SPEAKER_ORDER, gain=native.SPEAKER_GAIN):
        """CUDA int16 (n_streams, speaker_sample_count(tick_count(), decim)): what the ticks of ticks() will sound like on the
        machine, before anything is encoded -- the player's pulses through a CIC decimator, at speaker_rate(decim) samples a
        second (include/iivision.h f13).  Asynchronous on torch's current stream."""
        n = self.tick_count()
        pcm, _ = native.speaker_pcm(self.ticks()[:, :n].contiguous(), None, decim, order, gain)
        return pcm[:, :native.speaker_sample_count(n, decim)]

    def audio_stream(self, stream=0) -> Iterator[int]:
        """audio.Audio.audio_stream: the samples -15 .. 16 of one stream"""
        if self.n_streams == 0 or self.n_frames == 0:
            return
        t = self.ticks()[stream, :self.tick_count()].cpu().numpy().astype(np.int64)
        yield from ((t - 34) // 2).tolist()


class Audio:
    """audio.Audio (transcoder/audio.py:9-107): Audio(filename, bitrate=14700, normalization=None).audio_stream()
    yields one int -15 .. 16 per tick; `normalization` falsy = computed from the file (Audio._normalization)."""

    def __init__(self, filename: str, bitrate: int = BITRATE, normalization: float = None):
        self.filename = filename
        self._tick_range = [4, 66]
        self.sample_rate = float(bitrate)
        pcm, rate = read_wav(filename)
        self._array = ArrayAudio(pcm, rate, int(bitrate), normalization or None)
        self.normalization = float(self._array.normalization[0])

    def audio_stream(self) -> Iterator[int]:
        yield from self._array.audio_stream()
