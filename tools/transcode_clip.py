"""End to end on one GPU, everything on the device: RGB frames -> memory maps (f3, csrc/iiv_ingest.hip) ->
Movie-paced encode (the hot path + f1: prologue / greedy kernels driven by stream_batch.MovieClock) -> player byte
stream (f2, csrc/iiv_a2m.hip) -> an .a2m file.  What the reference's `main.py in.mp4 out.a2m` does between its decoder
and its output file (transcoder/main.py, movie.py:56-161).  The speaker duty cycle of every opcode comes from the clip's
audio (`--audio clip.wav`, or `--pcm pcm.npy --rate R`: csrc/iiv_audio.hip, transcoder/audio.py), and the movie ends where
the audio or the frames run out, whichever is first (movie.py:67-74); without audio every opcode carries the same duty
cycle (`--tick`, 4..66 even: movie.py:104-107).

    python tools/transcode_clip.py --frames clip.npy --out clip.a2m --dbg /path/to/player/iivision.dbg
    python tools/transcode_clip.py --synthetic 90 --out /tmp/bars.a2m            # a moving test card
    python tools/transcode_clip.py --frames clip.npy --audio clip.wav --out clip.a2m
    python tools/transcode_clip.py --yuv clip.yuv --size 640x480 --out clip.a2m   # ffmpeg -f rawvideo -pix_fmt yuv420p

--palette MONO: the stream is encoded for a monochrome monitor: frames are taken at one pixel per dot
(560x192 for DHGR, 280x192 for HGR; anything else is resized to that), converted by csrc/iiv_mono.hip and priced by
palette.MonoPalette.diff_matrix().
--frames: uint8 array (n, h, w, 3) of any size (1 <= h, w <= 8192): frames that are not 280x192 are resized on the
device, byte for byte as the reference's Image.resize((280, 192), LANCZOS) (frame_grabber.py:75,100; csrc/iiv_resize.hip);
a (n, 192, 280, 3) array is taken as it is.
--yuv FILE --size WxH [--pix-fmt yuv420p|nv12] [--yuv-matrix bt601|bt709|jpeg]: raw 4:2:0 frames as `ffmpeg -f rawvideo` writes
them (yuv420p: the Y plane, then Cb, then Cr; nv12: the Y plane, then Cb and Cr interleaved), converted inside the device resize
(include/iivision.h f11); a file that is not a whole number of frames is an error.  --dbg: the player's cc65 debug file, from which the opcode entry points are read exactly as
opcodes._parse_symbol_table does (opcodes.py:168-185); without it the stream is written with placeholder addresses
and is NOT playable (the tool says so).  --fourth / --joint: the two optional quality modes.
--preview FILE.npy: also write what the stream puts on the screen, a uint8 array (frames, 192, 560, 3): the screen as it stands
after each source frame's opcodes, drawn on the device from the encoder's own screen memory in the clip's palette
(csrc/iiv_render.hip).  The .a2m bytes are the same with and without it.
--quality FILE.json: also measure that screen against the frame that went into the ingest (after any resize: 280 wide, 560
for --palette MONO in DHGR), on the device (csrc/iiv_render_error.hip): per source frame the nine exact sums of
squared differences [level][channel] -- per dot, per quad of four dots, per unit of sixteen -- and the overall PSNR of each
level (screen.psnr).  The .a2m bytes and the --preview array are the same with and without it.
--fit letterbox / crop (with --sar N:D, --fill R,G,B): a source that is not 4:3 on display keeps its shape -- whole, between bars of
the fill colour, or cropped to its centred 4:3 part (frame_grabber.fit_geometry) -- instead of being stretched over the
screen as the reference does; --preview shows it and --quality measures against the fitted frame, the one the ingest saw.
--preview-audio FILE.wav: also write what the stream's ticks sound like on the machine, 16-bit mono PCM at 44 369 Hz: the speaker's
pulses, ACKs included, through the default CIC decimator (csrc/iiv_speaker.hip; tools/play_a2m.py --audio gives the
same samples from the file and takes the filter's parameters).  The .a2m bytes are the same with and without it.
--temporal LO,HI: the temporal hold in front of the conversion (csrc/iiv_temporal.hip): a pixel within LO of the value
held for it keeps the held bytes from frame to frame, one more than HI away takes the source's, one between moves part of the way;
0,0 is the identity.  With --quality the JSON gains, per frame, the pixels held, blended and passed.  --synthetic-noise A adds
uniform noise of -A..A (seeded by --seed, clamped) to the test card: the still parts of a noisy source are what the hold is for.
--levels auto[:LO,HI] / --levels BLACK,WHITE, --gamma G, --brightness B, --contrast C, --saturation S: picture levels behind the
resize and in front of the hold (csrc/iiv_levels.hip; frame_grabber.Levels).  auto takes the black and white points
from the clip's own luma histogram, at most LO and HI millionths of the pixels below and above them (5000,5000 by default: the
0.5th and 99.5th percentiles); BLACK,WHITE gives them.  Any one of the five options turns the stage on; none of them leaves every
byte as it was.  With --quality the JSON gains a "picture_levels" block: the points and parameters in use.  --synthetic-range LO,HI
squeezes the test card into LO..HI: a clip graded into 16..235, or a washed-out transfer, is what --levels auto is for.
--denoise LO,HI, --sharpen AMOUNT[,THRESHOLD], --blur SX[,SY]: the spatial filter behind the levels and in front of the hold
(csrc/iiv_filter.hip; frame_grabber.Spatial).  A pixel is compared with a 5 x 5 blur of its neighbourhood -- Gaussian,
sigmas SX and SY in pixels (SY = SX when left out); without --blur the binomial (1, 4, 6, 4, 1) / 16 on both axes --; where the
largest channel difference is at most LO the pixel takes the blur's value, above HI it is left alone, between it moves part of the
way (denoise); where it is above THRESHOLD (by default HI, or 0 without --denoise) the difference is amplified by AMOUNT / 256
(sharpen, an unsharp mask; AMOUNT 0..1024).  Any one of the three turns the stage on; none of them leaves every byte as it was."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
import numpy as np  # noqa: E402


def test_card(n, width=280):
    """n frames (192, width, 3): colour bars drifting over a grey ramp (width 560: the same card at one pixel per DHGR dot)"""
    y, x = np.mgrid[0:192, 0:width]
    x = x * 280 // width
    bars = np.array([[255, 255, 255], [255, 255, 0], [0, 255, 255], [0, 255, 0], [255, 0, 255], [255, 0, 0], [0, 0, 255], [0, 0, 0]], np.uint8)
    out = np.empty((n, 192, width, 3), np.uint8)
    for f in range(n):
        out[f] = bars[((x + 3 * f) // 35) % 8]
        out[f, 128:] = ((x[128:] + y[128:] - 2 * f) % 256)[..., None]
    return out


def squeeze(frames, lo, hi):
    """the frames' 0..255 taken linearly into lo..hi, rounded half up; (0, 255) returns the frames as they are"""
    if (lo, hi) == (0, 255):
        return frames
    return ((frames.astype(np.int64) * (2 * (hi - lo)) + 255) // 510 + lo).astype(np.uint8)


def add_noise(frames, amplitude, seed):
    """uniform noise of -amplitude..amplitude on every byte, clamped; amplitude 0 returns the frames as they are"""
    if amplitude == 0:
        return frames
    noise = np.random.default_rng(seed).integers(-amplitude, amplitude + 1, frames.shape)
    return np.clip(frames.astype(np.int64) + noise, 0, 255).astype(np.uint8)


def read_yuv(path, size, pix_fmt):
    """A raw 4:2:0 file -> (y, u, v) uint8 arrays, y (n, h, w), u / v (n, ch, cw): views of the file's bytes, NV12's interleaved"""
    try:
        w, h = (int(v) for v in size.lower().split("x"))
    except ValueError:
        raise SystemExit("--size: WxH, e.g. 640x480 (got %r)" % size)
    if w < 1 or h < 1:
        raise SystemExit("--size: WxH, both at least 1 (got %r)" % size)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    frame = h * w + 2 * ch * cw
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size == 0 or raw.size % frame:
        raise SystemExit("%s holds %d bytes: not a whole number of %dx%d %s frames of %d bytes (%d frames and %d bytes over)" % (
            path, raw.size, w, h, pix_fmt, frame, raw.size // frame, raw.size % frame))
    raw = raw.reshape(-1, frame)
    y = raw[:, :h * w].reshape(-1, h, w)
    if pix_fmt == "nv12":
        uv = raw[:, h * w:].reshape(-1, ch, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    return y, raw[:, h * w:h * w + ch * cw].reshape(-1, ch, cw), raw[:, h * w + ch * cw:].reshape(-1, ch, cw)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", help=".npy file, uint8 (n, h, w, 3); resized to 280x192 on the device when not that size")
    ap.add_argument("--synthetic", type=int, default=0, help="instead of --frames: this many frames of a moving test card")
    ap.add_argument("--yuv", help="instead of --frames: raw 4:2:0 frames (ffmpeg -f rawvideo), with --size")
    ap.add_argument("--size", help="with --yuv: WxH of its frames")
    ap.add_argument("--pix-fmt", choices=["yuv420p", "nv12"], default="yuv420p", help="with --yuv: the file's layout")
    ap.add_argument("--yuv-matrix", choices=["bt601", "bt709", "jpeg"], default="bt601", help="with --yuv: YCbCr -> RGB (frame_grabber.YUV_MATRICES)")
    ap.add_argument("--fit", choices=["stretch", "letterbox", "crop"], default="stretch",
                    help="how a source that is not 4:3 goes onto the 4:3 screen (frame_grabber.fit_geometry): stretched over it (the "
                         "reference), whole between bars, or its centred 4:3 part; --synthetic is then a 16:9 card, 192x341")
    ap.add_argument("--sar", default="1:1", metavar="N:D", help="with --fit: the source's pixel aspect ratio")
    ap.add_argument("--fill", default="0,0,0", metavar="R,G,B", help="with --fit letterbox: the bars' colour")
    ap.add_argument("--out", required=True)
    ap.add_argument("--mode", choices=["DHGR", "HGR"], default="DHGR")
    ap.add_argument("--palette", choices=["NTSC", "IIGS", "MONO"], default="NTSC",
                    help="MONO: a monochrome monitor -- one source pixel per dot (560x192 DHGR, 280x192 HGR), dot-level distances (DESIGN.md 12)")
    ap.add_argument("--dither", default="diffusion",
                    help='"diffusion" (Floyd-Steinberg), the amplitude 0..255 of the ordered dither, or an error-diffusion kernel by name: '
                         'floyd-steinberg, jarvis, stucki, atkinson, burkes, sierra, sierra-2, sierra-lite, buckels (frame_grabber.DIFFUSION_KERNELS), or "direct": per screen row the bytes whose rendered dots '
                         'are nearest the frame (DESIGN.md 22)')
    ap.add_argument("--amplitude", type=int, default=0, help='with --dither direct: the ordered dither 0..255 added to its target')
    ap.add_argument("--dbg", help="player/iivision.dbg (opcode entry points)")
    ap.add_argument("--tick", type=int, default=34, help="without audio: speaker duty cycle of every opcode (4..66, even)")
    ap.add_argument("--audio", help="16-bit PCM .wav: the clip's audio track")
    ap.add_argument("--pcm", help="instead of --audio: .npy int16 (n_frames, channels) or (n_frames,), at --rate Hz")
    ap.add_argument("--rate", type=int, help="sample rate of --pcm")
    ap.add_argument("--normalization", type=float, default=None,
                    help="Audio(normalization=); default: computed from the audio's first 10 MiB (audio.py:60-78)")
    ap.add_argument("--fourth", action="store_true", help="IIV_OPT_FOURTH_OFFSET (not the reference's stream)")
    ap.add_argument("--joint", action="store_true", help="IIV_CONTENT_JOINT (not the reference's stream)")
    ap.add_argument("--preview", metavar="FILE.npy", help="also write the screen after each source frame's opcodes: uint8 (frames, 192, 560, 3)")
    ap.add_argument("--preview-audio", metavar="FILE.wav", help="also write the PCM the stream's ticks play: 16-bit mono at 44 369 Hz")
    ap.add_argument("--quality", metavar="FILE.json",
                    help="also write, per source frame, the screen's squared error against the ingest's input frame (nine sums) and three PSNRs")
    ap.add_argument("--seed", type=int, default=1, help="random.seed / np.random.seed of the encoder's two nonce streams")
    ap.add_argument("--temporal", metavar="LO,HI", help="the temporal hold in front of the conversion: 0 <= LO <= HI <= 255 (DESIGN.md 30)")
    ap.add_argument("--synthetic-noise", type=int, default=0, metavar="A",
                    help="with --synthetic: uniform noise of -A..A on the test card, seeded by --seed (0: the card as it is)")
    ap.add_argument("--levels", metavar="auto[:LO,HI] | BLACK,WHITE", help="picture levels: the black and white points, found or given (DESIGN.md 31)")
    ap.add_argument("--gamma", type=float, default=None, help="picture levels: gamma, above 1 lifts the mid-tones (1: none)")
    ap.add_argument("--brightness", type=float, default=None, help="picture levels: added to every channel, in levels (0: none)")
    ap.add_argument("--contrast", type=float, default=None, help="picture levels: slope about mid-grey (1: none)")
    ap.add_argument("--saturation", type=float, default=None, help="picture levels: 0 grey, 1 none, up to 4")
    ap.add_argument("--synthetic-range", metavar="LO,HI", help="with --synthetic: the test card squeezed into LO..HI")
    ap.add_argument("--denoise", metavar="LO,HI", help="spatial filter: pull a pixel within LO of its neighbourhood's blur to it, leave one above HI (DESIGN.md 33)")
    ap.add_argument("--sharpen", metavar="AMOUNT[,THRESHOLD]", help="spatial filter: unsharp mask, AMOUNT / 256 (0..1024) of the difference above THRESHOLD")
    ap.add_argument("--blur", metavar="SX[,SY]", help="spatial filter: the Gaussian sigmas of the blur in pixels (default: binomial taps)")
    a = ap.parse_args()
    spatial_args = None
    if a.denoise is not None or a.sharpen is not None or a.blur is not None:
        spatial_args = {}
        try:
            if a.denoise is not None:
                spatial_args["denoise"] = tuple(int(v) for v in a.denoise.split(","))
                if len(spatial_args["denoise"]) != 2 or not 0 <= spatial_args["denoise"][0] <= spatial_args["denoise"][1] <= 255:
                    raise ValueError
            if a.sharpen is not None:
                sharpen = tuple(int(v) for v in a.sharpen.split(","))
                if len(sharpen) == 1:
                    sharpen += (spatial_args["denoise"][1] if a.denoise is not None else 0,)
                if len(sharpen) != 2 or not 0 <= sharpen[0] <= 1024 or not spatial_args.get("denoise", (0, 0))[1] <= sharpen[1] <= 255:
                    raise ValueError
                spatial_args["sharpen"] = sharpen
            if a.blur is not None:
                blur = tuple(float(v) for v in a.blur.split(","))
                if len(blur) == 1:
                    blur += blur
                if len(blur) != 2 or not all(0 <= v < float("inf") for v in blur):
                    raise ValueError
                spatial_args["blur"] = blur
        except ValueError:
            ap.error("--denoise LO,HI with 0 <= LO <= HI <= 255; --sharpen AMOUNT[,THRESHOLD] with 0..1024 and HI <= THRESHOLD <= 255; "
                     "--blur SX[,SY] with sigmas >= 0")
    levels_args = None
    if a.levels is not None or any(v is not None for v in (a.gamma, a.brightness, a.contrast, a.saturation)):
        levels_args = dict(gamma=1.0 if a.gamma is None else a.gamma, brightness=0 if a.brightness is None else a.brightness,
                           contrast=1.0 if a.contrast is None else a.contrast, saturation=1.0 if a.saturation is None else a.saturation)
        try:
            if a.levels is None:
                pass
            elif a.levels == "auto":
                levels_args["auto"] = (5000, 5000)
            elif a.levels.startswith("auto:"):
                levels_args["auto"] = tuple(int(v) for v in a.levels[5:].split(","))
                if len(levels_args["auto"]) != 2 or not all(0 <= v <= 500000 for v in levels_args["auto"]):
                    raise ValueError
            else:
                points = tuple(int(v) for v in a.levels.split(","))
                if len(points) != 2 or not 0 <= points[0] < points[1] <= 255:
                    raise ValueError
                levels_args["black"], levels_args["white"] = points
        except ValueError:
            ap.error("--levels auto, auto:LO,HI with 0..500000 each, or BLACK,WHITE with 0 <= BLACK < WHITE <= 255")
        if not (levels_args["gamma"] > 0 and levels_args["contrast"] >= 0 and -255 <= levels_args["brightness"] <= 255
                and 0 <= levels_args["saturation"] <= 4):
            ap.error("--gamma above 0, --contrast at least 0, --brightness -255..255, --saturation 0..4")
    synthetic_range = (0, 255)
    if a.synthetic_range:
        try:
            synthetic_range = tuple(int(v) for v in a.synthetic_range.split(","))
            if len(synthetic_range) != 2 or not 0 <= synthetic_range[0] < synthetic_range[1] <= 255 or not a.synthetic:
                raise ValueError
        except ValueError:
            ap.error("--synthetic-range LO,HI with 0 <= LO < HI <= 255, with --synthetic")
    temporal = None
    if a.temporal:
        try:
            temporal = tuple(int(v) for v in a.temporal.split(","))
            if len(temporal) != 2 or not 0 <= temporal[0] <= temporal[1] <= 255:
                raise ValueError
        except ValueError:
            ap.error("--temporal LO,HI with 0 <= LO <= HI <= 255")
    if a.synthetic_noise < 0 or a.synthetic_noise > 255 or (a.synthetic_noise and not a.synthetic):
        ap.error("--synthetic-noise: 0..255, with --synthetic")
    if a.tick < 4 or a.tick > 66 or a.tick % 2:
        ap.error("--tick: 4..66, even")
    if bool(a.frames) + bool(a.synthetic) + bool(a.yuv) != 1:
        ap.error("one of --frames / --synthetic / --yuv")
    if bool(a.yuv) != bool(a.size):
        ap.error("--yuv needs --size WxH (and --size goes with --yuv)")
    if a.audio and a.pcm:
        ap.error("one of --audio / --pcm")
    if bool(a.pcm) != bool(a.rate):
        ap.error("--pcm needs --rate (and --rate goes with --pcm)")
    try:
        sar = tuple(int(v) for v in a.sar.split(":"))
        fill = tuple(int(v) for v in a.fill.split(","))
        if len(sar) != 2 or min(sar) < 1 or len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
            raise ValueError
    except ValueError:
        ap.error("--sar N:D with positive integers, --fill R,G,B with 0..255")

    import torch
    import _iiv_native as native
    import a2m
    import audio
    import frame_grabber
    import palette
    import stream_batch
    import video_mode

    mode = native.DHGR if a.mode == "DHGR" else native.HGR
    pal_id = palette.Palette[a.palette]
    rgb = read_yuv(a.yuv, a.size, a.pix_fmt) if a.yuv else np.load(a.frames) if a.frames else test_card(a.synthetic, 341 if a.fit != "stretch" else native.MONO_SIZE[mode][1] if pal_id == palette.Palette.MONO else 280)
    if a.synthetic:
        rgb = add_noise(squeeze(rgb, *synthetic_range), a.synthetic_noise, a.seed)
    t0 = time.perf_counter()
    hold = dict(temporal=temporal) if temporal is not None else {}
    if levels_args is not None:
        hold["levels"] = frame_grabber.Levels(**levels_args)
    if spatial_args is not None:
        hold["spatial"] = frame_grabber.Spatial(**spatial_args)
    grab = frame_grabber.ArrayFrameGrabber(rgb, video_mode.VideoMode[a.mode], pal_id,
                                           dither=int(a.dither) if a.dither.isdigit() else a.dither, resize=True,
                                           amplitude=a.amplitude, yuv_matrix=a.yuv_matrix, fit=a.fit, sar=sar, fill=fill, **hold)
    main_maps, aux_maps = grab.memory_maps()                       # (n, 32, 256) on the device
    dm = palette.diff_matrix(pal_id)                               # CIE2000 of the palette's colours; MONO: the dot distance
    table = native.build_table(mode, dm, True)
    store = native.build_store_table(mode, dm)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    batch = stream_batch.StreamBatch(mode, table, store, 1, seeds=[(a.seed, a.seed)], dm=dm, joint_content=a.joint, fourth_offset=a.fourth,
                                     input_frame_rate=grab.input_frame_rate)
    n = int(main_maps.shape[0])
    au = None
    if a.audio or a.pcm:
        if a.audio:
            au = audio.Audio(a.audio, normalization=a.normalization)._array
        else:
            au = audio.ArrayAudio(np.load(a.pcm), a.rate, normalization=a.normalization)
        audio_ticks = au.ticks()                                   # (1, n_ticks) on the device
        max_ticks = au.tick_count()
    else:
        max_ticks = None
    frames_main, frames_aux = main_maps[None], aux_maps[None] if aux_maps is not None else None
    if a.preview or a.quality:
        # the same schedule one source frame per call (MovieClock continues a movie across calls), the screen drawn and
        # measured behind each
        parts, segs, shots, sums, left = [], [], [], [], max_ticks
        ref = grab.ingest_frames() if a.quality else None
        for _ in range(n):
            if left is None or left > 0:
                o, s = batch.encode_frames(frames_main, frames_aux, 1, max_ticks=left)
                parts.append(o)
                segs += s
                left = None if left is None else left - int(o.shape[1])
            if a.preview:
                shots.append(batch.screens_rgb(pal_id))     # (the audio has run out: the screen stays as it is)
            if a.quality:
                sums.append(batch.screens_error(ref[len(sums):len(sums) + 1], pal_id))
        ops = torch.cat(parts, dim=1)
        batch.enc.check()
        if a.preview:
            np.save(a.preview, torch.cat(shots).cpu().numpy())
        if a.quality:
            import json
            import screen
            host = np.stack([t.cpu().numpy()[0] for t in sums])                   # (frames, 3, 3) uint64
            db = [screen.psnr(host, level)[1] for level in range(3)]
            per_frame = [{"frame": i, "sums": [[int(v) for v in row] for row in host[i]],
                          "psnr_db": [float(db[level][i]) for level in range(3)]} for i in range(n)]
            report = {"mode": a.mode, "palette": a.palette, "ref_width": int(ref.shape[2]), "levels": ["dot", "quad", "unit"],
                      "channels": ["R", "G", "B"], "frames": per_frame}
            if temporal is not None:
                report["temporal"] = {"lo": temporal[0], "hi": temporal[1], "counts": ["held", "blended", "passed"]}
                for entry, c in zip(per_frame, grab.temporal_counts()):
                    entry["temporal"] = [int(v) for v in c]
            if levels_args is not None:
                lv = grab.levels_report()
                report["picture_levels"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in lv.items()}
            with open(a.quality, "w") as f:
                json.dump(report, f, indent=1)
            print("screen against source, mean PSNR over %d frames: dot %.2f dB, quad %.2f dB, unit %.2f dB -> %s" % (
                n, *(float(np.mean(d)) for d in db), a.quality))
    else:
        ops, segs = batch.encode_frames(frames_main, frames_aux, n, max_ticks=max_ticks)
        batch.enc.check()
    if a.dbg:
        addr = a2m.OpcodeAddresses.from_debug_file(a.dbg)
    else:
        print("no --dbg: placeholder opcode addresses -- the stream has the right layout but is NOT playable", file=sys.stderr)
        addr = a2m.OpcodeAddresses.placeholder()
    if au is None:
        ticks = torch.full((1, ops.shape[1]), a.tick, dtype=torch.uint8, device="cuda")
    else:
        ticks = audio_ticks[:, :ops.shape[1]]                      # opcode k carries tick k (movie.py:67-111)
    stream = a2m.emit_stream(mode, ops, ticks, addr)
    if a.preview_audio:
        pcm, counts = native.speaker_pcm(ticks.contiguous())
        audio.write_wav(a.preview_audio, pcm[0, :counts[0]].cpu().numpy(), audio.speaker_rate())
    data = stream[0].cpu().numpy().tobytes()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    with open(a.out, "wb") as f:
        f.write(data)
    n_ops = int(ops.shape[1])
    distinct = np.mean([len(set(r[2:6])) for r in ops[0].cpu().numpy().tolist()])
    if au is not None:
        print("audio: %d ticks at %d Hz from %d frames at %d Hz (%d channels, normalization %.6g); the movie ends with the %s" % (
            max_ticks, au.bitrate, au.n_frames, au.rate, au.channels, au.normalization[0],
            "audio" if n_ops >= max_ticks else "frames"))
    print("%d frames (%s, %s palette, dither %s) -> %d opcodes (%.2f distinct offsets each), %d generators -> %d bytes in %s" % (
        n, a.mode, a.palette, a.dither, n_ops, distinct, len(stream_batch.merge_generators(segs)), len(data), a.out))
    print("tables + ingest %.2f s, encode + emit %.3f s = %.0f frames/s for this one clip (many clips at once: bench.py)" % (
        t1 - t0, t2 - t1, n / (t2 - t1)))
    batch.close()


if __name__ == "__main__":
    main()
