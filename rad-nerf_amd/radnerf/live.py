"""Live mode: render from an audio stream -- the loop of the reference's nerf/asr.py (run_step, get_next_feat) and nerf/gui.py:184-188,
560-563 over this tree's classes.

    python -m radnerf.live data/obama --workspace trial -O --pose clip.json --asr_weights w2v.pth --wav intro.wav --video
    arecord -f S16_LE -r 16000 -c 1 -t raw | python -m radnerf.live ... --pcm - --raw_out - --realtime | ffplay -f rawvideo ...

Audio arrives in chunks of 320 samples (20 ms).  `l` zero chunks stand in front; whenever l + m + r chunks are held, that one window
goes through the wav2vec2 model (radnerf/asr.py, RN_ASR as everywhere else), rows l .. T - r of its logits go into a ring of
ring_windows * m rows, and the last l + r chunks stay for the next window.  Every video frame pushes two chunks and reads the next
attention window [8, C, 16] out of the ring: entry e of frame k is slice s = k - 4 + e, rows ring_rows - 8 + 2 s .. + 15 (mod
ring_rows), zeros for s < 0 -- get_next_feat's `front` / `tail` walk as a closed form.  The reader starts warm_up_chunks = m + r + 14
chunks behind the stream: that is the algorithmic latency, warm_up_chunks / 50 seconds.

LiveASR     the held samples, the ring and the window per frame.  On a GPU the ring is two copy kernels (rn_asr_ring_push,
            rn_asr_ring_window) and nothing is read back; on a CPU module the same in plain torch (the host logic without a GPU).
            tail="reference": the reference to the letter -- the terminal window's rows are never written (asr.py:220), so the
            last frames read what the ring held before; a slice is a view of the ring, read anew by every frame that holds it,
            except the slice that wraps the ring's end, which is a copy made when it first enters a window (asr.py:165-176).  tail="flush" (default, a stated deviation): the terminal window's rows
            are written with 16 zero rows behind them and slices past M // 2 are zeros, so frame k's window equals
            get_audio_features(features_from_samples(x), 2, k) for every k and a live render of a .wav is the clip --aud_wav
            renders.  It needs ring_windows * m >= 2 m + r + 48 rows (the unread frames' rows, one window and the zero tail must
            not meet); the defaults pass (200 >= 158).
schedule    the loop: warm-up pushes, then per frame two pushes and one window; finish() when the source ends, then the frames
            that are left.
LiveScene   ClipScene whose audio comes from a LiveASR: the same frame dict, the same ray_source path.
main        the command line: --wav FILE or --pcm - (raw s16le 16 kHz mono); results/<name>.npy, --video, --raw_out FILE|-,
            --realtime.  --wav FILE --resample takes any PCM or float .wav, --pcm - --pcm_rate R --pcm_format F --pcm_channels C any
            raw stream: resampled_chunks pulls 20 ms source blocks through a resample.Resampler on the device and hands the loop
            the same chunks of 320 samples at 16 kHz, (W + 1) / R seconds later (the filter's right wing).

Not built: microphone capture, playback, the text decode, the GUI.
"""
import os
import sys
import time

import numpy as np
import torch

from .asr import CHUNK, MAX_STEPS, SAMPLE_RATE, frames_of
from .clip import ClipScene

CHUNK_RATE = SAMPLE_RATE // CHUNK          # 50 chunks per second
UNBOUNDED = 0xFFFFFFFF                     # n_slices while the stream is open
ZERO_TAIL = 16                             # zero rows behind the terminal window (tail="flush")


def check_schedule(l, m, r, ring_windows=4, tail="flush"):
    """ValueError for a schedule the live loop cannot run; -> (window chunks, ring rows)."""
    l, m, r, ring_windows = int(l), int(m), int(r), int(ring_windows)
    if l < 0 or r < 0 or m < 1 or ring_windows < 1:
        raise ValueError(f"LiveASR: l, m, r = {l}, {m}, {r}, ring_windows = {ring_windows} (l, r >= 0; m, ring_windows >= 1)")
    if tail not in ("flush", "reference"):
        raise ValueError(f"LiveASR: tail = {tail!r} is not 'flush' or 'reference'")
    size = l + m + r
    if size - 1 > MAX_STEPS:
        raise ValueError(f"LiveASR: a window of l + m + r = {size} chunks gives {size - 1} steps; the model's kernels take at most {MAX_STEPS}")
    rows = ring_windows * m
    if rows < 16:
        raise ValueError(f"LiveASR: a ring of ring_windows * m = {rows} rows is shorter than one 16-row slice")
    if tail == "flush" and rows < 2 * m + r + 48:
        raise ValueError(f"LiveASR: tail='flush' needs ring_windows * m >= 2 m + r + 48 = {2 * m + r + 48} rows, got {rows} "
                         f"(raise ring_windows, or tail='reference')")
    return size, rows


class LiveASR:
    def __init__(self, model, l=10, m=50, r=10, ring_windows=4, tail="flush"):
        """model: a Wav2Vec2CTC; everything lives on its device and is allocated here, once."""
        self.size, self.ring_rows = check_schedule(l, m, r, ring_windows, tail)
        self.model, self.l, self.m, self.r, self.ring_windows, self.tail = model, int(l), int(m), int(r), int(ring_windows), tail
        self.device = model.t0.device
        self.C = int(model.vocab_size)
        self.warm_up_chunks = self.m + self.r + 8 + 2 * 3        # asr.py:112: mid + right + window + attention
        f32 = dict(dtype=torch.float32, device=self.device)
        self.held = torch.zeros(self.size * CHUNK, **f32)        # the held chunks, l zero chunks first
        self._keep = torch.empty((self.l + self.r) * CHUNK, **f32)
        self.held_samples = self.l * CHUNK
        self._pending = torch.zeros(0, **f32)                    # samples short of a chunk
        self.ring = torch.zeros(self.ring_rows, self.C, **f32)
        self.logits = torch.empty(max(self.size - 1, 1), self.C, **f32)
        self.window = torch.empty(8, self.C, 16, **f32)
        self._copies = {}                                        # tail="reference": slice -> its copy, for the slices that wrap the ring
        self._next_frame = 0
        self._hip = self.device.type == "cuda"
        self._workspace = None
        if self._hip:
            n = model.workspace_bytes(1, self.size * CHUNK)
            self._workspace = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)
        self.pushed_chunks = 0          # chunks of the stream so far, a short last one included
        self.windows_run = 0
        self.rows_written = 0           # kept rows so far (tail="flush": row i of the stream sits at ring row i % ring_rows)
        self._zero_rows = 0
        self._slot = 0                  # tail="reference": the next window's ring slot (asr.py:221-224)
        self.finished = False

    # ------------------------------------------------------------------------------------------------------------ the stream
    def push(self, samples):
        """Any number of float32 samples in [-1, 1); they are cut into chunks of 320 here, what is left over waits for the next
        call (or for finish(), which takes it as the stream's short last chunk)."""
        if self.finished:
            raise RuntimeError("LiveASR.push: the stream was finished")
        x = torch.as_tensor(samples).to(self.device, torch.float32).reshape(-1)
        x = torch.cat([self._pending, x]) if self._pending.numel() else x
        at, whole = 0, x.numel() // CHUNK
        while whole > 0:
            n_held = self.held_samples // CHUNK
            take = min(whole, self.size - n_held)
            self.held[self.held_samples:self.held_samples + take * CHUNK].copy_(x[at:at + take * CHUNK])
            self.held_samples += take * CHUNK
            self.pushed_chunks += take
            at += take * CHUNK
            whole -= take
            if n_held + take == self.size:
                self._run_window(terminal=False)
        self._pending = x[at:].clone()

    def finish(self):
        """The stream has ended: samples short of a chunk become its short last chunk (asr.py:304-306), a window that this
        completes runs, and then the terminal window over whatever is held."""
        if self.finished:
            return
        n = self._pending.numel()
        if n:
            self.held[self.held_samples:self.held_samples + n].copy_(self._pending)
            self.held_samples += n
            self.pushed_chunks += 1
            self._pending = self._pending[:0]
            if -(-self.held_samples // CHUNK) == self.size:
                self._run_window(terminal=False)
        self.finished = True
        if self.held_samples > 0:
            self._run_window(terminal=True)

    def _model_pass(self, S, T):
        win = self.held[:S].unsqueeze(0)
        out = self.logits[:T]
        with torch.no_grad():
            if self.model._hip_usable(win):
                self.model.forward_hip(win, out=out.view(1, T, self.C), workspace=self._workspace)
            else:
                out.copy_(self.model.forward_torch(win)[0])
        self.windows_run += 1
        return out

    def _run_window(self, terminal):
        S = self.held_samples
        T = frames_of(self.model.config, S)
        write = not terminal or self.tail == "flush"           # asr.py:220: the terminal window's rows are not recorded
        if write:
            left, right, zeros = 0, 0, ZERO_TAIL if terminal else 0
            if T >= 1:
                self._model_pass(S, T)
                right = T if terminal else min(T, T - self.r + 1)
                left = min(self.l, right)
            first = self.rows_written % self.ring_rows if self.tail == "flush" else self._slot * self.m
            self._ring_push(T, left, right, first, zeros)
            self.rows_written += right - left
            self._zero_rows = zeros
            self._slot = (self._slot + 1) % self.ring_windows
        if not terminal:                                        # asr.py:209-210: the last l + r chunks stay
            n = S - self.m * CHUNK
            self._keep[:n].copy_(self.held[self.m * CHUNK:S])
            self.held[:n].copy_(self._keep[:n])
            self.held_samples = n

    # -------------------------------------------------------------------------------------------------------------- the ring
    def _ring_push(self, T, left, right, first, zeros):
        if right - left + zeros == 0:
            return
        if self._hip:
            import radnerf_hip as hip
            hip.call("rn_asr_ring_push", hip.ptr(self.logits), max(T, 0), self.C, left, right, hip.ptr(self.ring), self.ring_rows, first, zeros,
                     hip.stream())
            return
        rows = (first + torch.arange(right - left + zeros, device=self.device)) % self.ring_rows
        self.ring[rows[:right - left]] = self.logits[left:right]
        self.ring[rows[right - left:]] = 0.0

    @property
    def n_slices(self):
        return self.rows_written // 2 + 1 if self.finished and self.tail == "flush" else UNBOUNDED

    @property
    def n_frames(self):
        """Frames of the whole stream; None while it is open.  tail="flush": M // 2 + 1 for M kept rows, the length of the
        feature file.  tail="reference": the frames the reference's loop draws until the step that finds the source empty."""
        if not self.finished:
            return None
        if self.tail == "flush":
            return self.rows_written // 2 + 1
        return max(0, -(-(self.pushed_chunks + 1 - self.warm_up_chunks) // 2))

    def frames_ready(self):
        """Frames whose window can be read now: every row they read has been written (tail="flush"), or the reference's schedule
        has reached them (tail="reference")."""
        if self.finished:
            return self.n_frames
        if self.tail == "flush":
            return 0 if self.rows_written < 14 else (self.rows_written - 14) // 2 + 1
        return max(0, (self.pushed_chunks - self.warm_up_chunks) // 2)

    def next_window(self, k):
        """Frame k's attention window [8, C, 16] on the model's device.  The buffer is reused: the next call overwrites it.
        tail="reference" hands the frames out in order, 0, 1, 2, ...: the reference keeps a slice as a VIEW of its ring
        (asr.py:166, the permute and the list keep it one), so every frame's torch.stack reads the ring's rows as they are then,
        but a slice that wraps the ring's end is a torch.cat (asr.py:169), a copy made when the slice first enters a window
        (slices 0 .. 3 at frame 0, slice k + 3 at frame k) and carried through the seven frames after.  Where the writer laps the
        reader the two differ, and both are kept here."""
        k = int(k)
        if k < 0:
            raise ValueError(f"LiveASR.next_window: frame {k}")
        if self.tail == "flush":
            if k >= self.frames_ready():
                raise RuntimeError(f"LiveASR.next_window: frame {k} is not ready ({self.frames_ready()} are): push more samples or finish()")
            if max(0, 2 * (k - 4) - 8) < self.rows_written + self._zero_rows - self.ring_rows:
                raise RuntimeError(f"LiveASR.next_window: frame {k}'s rows were overwritten: the reader fell more than a ring behind")
            return self._read_window(k, self.window)
        if k != self._next_frame:
            raise ValueError(f"LiveASR.next_window: tail='reference' hands the frames out in order; frame {self._next_frame} is next, not {k}")
        self._next_frame += 1
        self._read_window(k, self.window)                               # every slice as the ring holds it now
        for e in range(8):
            s = k - 4 + e
            if s >= 0 and (self.ring_rows - 8 + 2 * s) % self.ring_rows + 16 >= self.ring_rows:     # front >= tail: the copy
                if s in self._copies:
                    self.window[e].copy_(self._copies[s])
                else:
                    self._copies[s] = self.window[e].clone()
        for s in [s for s in self._copies if s < k - 3]:
            del self._copies[s]
        return self.window

    def _read_window(self, k, out):
        n_slices = self.n_slices
        if self._hip:
            import radnerf_hip as hip
            hip.call("rn_asr_ring_window", hip.ptr(self.ring), self.ring_rows, self.C, k, n_slices, hip.ptr(out), hip.stream())
            return out
        t = torch.arange(16, device=self.device)
        for e in range(8):
            s = k - 4 + e
            if 0 <= s < n_slices:
                out[e].copy_(self.ring[(self.ring_rows - 8 + 2 * s + t) % self.ring_rows].t())
            else:
                out[e].zero_()
        return out


def schedule(live, read_chunk):
    """The loop (asr.py:372-379, gui.py:184-188): warm-up pushes, then per frame two pushes and the frame; when read_chunk()
    comes back short or empty the stream is finished, and the frames that are left follow.  Yields the frame indices; the caller
    takes live.next_window(k) (or renders a LiveScene's frame k) before asking for the next."""
    def feed():
        if live.finished:
            return
        x = read_chunk()
        if len(x):
            live.push(x)
        if len(x) < CHUNK:
            live.finish()
    for _ in range(live.warm_up_chunks):
        feed()
    k = 0
    while True:
        feed()
        feed()
        if live.finished and k >= live.n_frames:
            return
        yield k
        k += 1


def chunks_of(samples):
    """read_chunk over an array of samples."""
    x = np.asarray(samples, dtype=np.float32).reshape(-1)
    at = [0]
    def read_chunk():
        out = x[at[0]:at[0] + CHUNK]
        at[0] += CHUNK
        return out
    return read_chunk


def pcm_chunks(stream):
    """read_chunk over a binary stream of raw s16le mono samples at 16 kHz: one blocking read of a chunk per call; the values are
    int16 / 32768, as read_wav gives them."""
    def read_chunk():
        raw = stream.read(2 * CHUNK)
        return np.frombuffer(raw[:len(raw) & ~1], dtype="<i2").astype(np.float32) / np.float32(32768)
    return read_chunk


def block_reader(stream, rate, format, channels):
    """read_source for resampled_chunks over a binary stream: one blocking read of a 20 ms block, round(rate / 50) frames, per call."""
    from .resample import FORMATS
    nbytes = max(1, int(round(rate / CHUNK_RATE))) * int(channels) * FORMATS[format]
    return lambda: stream.read(nbytes)


def resampled_chunks(read_source, resampler):
    """read_chunk over a source at any rate and format: read_source() gives the next raw block (bytes in the resampler's format;
    a short or empty block ends the source).  Blocks are pushed through the resampler until 320 output samples are ready and exactly
    320 are handed out; once the source has ended and been flushed, what is left goes out in whole chunks and then once short
    (possibly empty) -- the only short chunk, which schedule() reads as the end of the stream.  The samples stay on the resampler's
    device."""
    from .resample import FORMATS
    state = dict(ready=torch.zeros(0, dtype=torch.float32, device=resampler.device), ended=False)
    block = max(1, int(round(resampler.src / CHUNK_RATE))) * resampler.channels * FORMATS[resampler.format]      # bytes of a whole block
    def read_chunk():
        while not state["ended"] and state["ready"].numel() < CHUNK:
            raw = read_source()
            got = [resampler.push(raw)] if len(raw) else []
            if len(raw) < block:
                state["ended"] = True
                got.append(resampler.flush())
            state["ready"] = torch.cat([state["ready"]] + got)
        out, state["ready"] = state["ready"][:CHUNK], state["ready"][CHUNK:]
        return out
    return read_chunk


class LiveScene(ClipScene):
    def __init__(self, model, clip, opt, device, live):
        """clip: the poses, eye values, intrinsics and background (its audio is not read); live: the LiveASR the windows come from."""
        att = int(getattr(opt, "att", 2))
        if att != 2:
            raise ValueError(f"LiveScene: --att {att} is not built for live mode: the ring hands out the 8-slice window of --att 2 only "
                             f"(--att 0 and --att 1 are refused)")
        if live.C != int(getattr(model, "audio_in_dim", live.C)):
            raise ValueError(f"LiveScene: the ASR model gives logits of width {live.C}, the audio net of this checkpoint takes {model.audio_in_dim}")
        self.live = live
        super().__init__(model, clip, opt, device)
        self.n_frames = 1 << 62         # no frame index is past the end of an open stream; its length is live.n_frames

    def _auds(self, i):
        return self.live.next_window(i)


# ------------------------------------------------------------------------------------------------------------------ command line
def _live_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m radnerf.live", add_help=False, allow_abbrev=False,
                                description="render a clip from an audio stream; every other flag is radnerf.cli's (a --test render)")
    p.add_argument("--wav", type=str, default="", help="16 kHz PCM16 .wav to stream; with --resample any PCM or float .wav")
    p.add_argument("--pcm", type=str, default="", help="'-': raw s16le 16 kHz mono on stdin, two chunks per frame (or a file / FIFO)")
    p.add_argument("--pcm_rate", type=int, default=SAMPLE_RATE, help="--pcm: the stream's sample rate; another than 16000 is resampled on the device")
    p.add_argument("--pcm_format", type=str, default="s16le", choices=("u8", "s16le", "s24le", "s32le", "f32le"), help="--pcm: the sample format")
    p.add_argument("--pcm_channels", type=int, default=1, help="--pcm: interleaved channels; the first is taken")
    p.add_argument("--raw_out", type=str, default="", help="FILE or '-': the frames as rgb24, written as they are produced")
    p.add_argument("--realtime", action="store_true", help="hold frame k back until k / video_fps seconds after the first")
    p.add_argument("--fps", type=int, default=CHUNK_RATE, help="audio chunks per second; only 50 (20 ms chunks) is built")
    p.add_argument("--ring_windows", type=int, default=4)
    p.add_argument("--tail", type=str, default="flush", choices=("flush", "reference"))
    p.add_argument("--no_npy", action="store_true", help="keep no frames for results/<name>.npy (an endless stream)")
    p.add_argument("--asr_weights", type=str, default="", help="state dict of Wav2Vec2ForCTC; nothing is fetched")
    p.add_argument("--asr_config", type=str, default="", help="the model's config.json (default: the large shape)")
    return p


def parse(argv=None):
    """argv -> opt: radnerf.cli's opt of a --test render plus the live flags.  Touches no GPU; errors end through argparse."""
    from . import cli
    from .asr import check_wav
    lp = _live_parser()
    lopt, rest = lp.parse_known_args(argv)
    if "-h" in rest or "--help" in rest:
        lp.print_help()
    opt = cli.parse(list(rest) + ["--test"])
    for k, v in vars(lopt).items():
        setattr(opt, k, v)
    if opt.wav and opt.pcm:
        lp.error("--wav and --pcm both name the audio source; give one")
    if not opt.wav and not opt.pcm:
        lp.error("an audio source is needed: --wav FILE or --pcm -")
    if opt.fps != CHUNK_RATE:
        lp.error(f"--fps {opt.fps}: the audio chunk rate is {CHUNK_RATE} per second (320 samples at 16 kHz); no other rate is built")
    if opt.att != 2:
        lp.error(f"--att {opt.att}: live mode hands out the 8-slice window of --att 2 only (--att 0 and --att 1 are refused)")
    if opt.aud or opt.aud_wav:
        lp.error("--aud / --aud_wav name a whole clip's audio; live mode takes --wav or --pcm")
    if not opt.pose:
        lp.error("--pose FILE (the transforms file of the clip's poses) is required")
    if not opt.asr_weights:
        lp.error("--asr_weights FILE (the state dict of Wav2Vec2ForCTC) is required: the model's weights are not fetched from anywhere")
    for flag in ("wav", "asr_weights", "asr_config"):
        if getattr(opt, flag) and not os.path.isfile(getattr(opt, flag)):
            lp.error(f"--{flag}: {getattr(opt, flag)} is not a file")
    if opt.pcm and opt.pcm != "-" and not os.path.exists(opt.pcm):
        lp.error(f"--pcm: {opt.pcm} does not exist")
    if not opt.pcm and (opt.pcm_rate, opt.pcm_format, opt.pcm_channels) != (SAMPLE_RATE, "s16le", 1):
        lp.error("--pcm_rate / --pcm_format / --pcm_channels describe the stream of --pcm; a --wav file describes itself")
    if opt.pcm_channels < 1:
        lp.error(f"--pcm_channels {opt.pcm_channels}: at least one channel")
    opt.pcm_resample = bool(opt.pcm) and (opt.pcm_rate, opt.pcm_format, opt.pcm_channels) != (SAMPLE_RATE, "s16le", 1)
    try:
        if opt.pcm_resample:
            from .resample import plan as resample_plan
            resample_plan(opt.pcm_rate)
        if opt.wav and opt.resample:
            from . import resample
            resample.plan(resample.check_audio(opt.wav)[0])
        elif opt.wav:
            check_wav(opt.wav)
    except ValueError as e:
        lp.error(f"{'--wav' if opt.wav else '--pcm_rate'}: {e}")
    try:
        check_schedule(opt.l, opt.m, opt.r, opt.ring_windows, opt.tail)
    except ValueError as e:
        lp.error(str(e))
    return opt


def main(argv=None, log=None, decode=None, stdin=None):
    """-> a dict of what was done: video (the .npy, or None), n_frames, avi, raw_out, latency, frame_ms."""
    opt = parse(argv)
    if log is None:
        log = (lambda *a: print(*a, file=sys.stderr)) if opt.raw_out == "-" else print
    from . import cli
    from .asr import Wav2Vec2CTC, read_wav
    from .checkpoint import load_checkpoint
    from .datafiles import load_clip
    from .output import FrameSink
    from .parallel import FrameParallelRenderer
    if not torch.cuda.is_available():
        raise RuntimeError("radnerf.live needs a GPU")
    device = torch.device("cuda", torch.cuda.current_device())
    model = cli._model(opt, device, log)
    path = cli._which_checkpoint(opt, log)
    if path is None:
        raise FileNotFoundError("radnerf.live needs a checkpoint (--ckpt latest found none)")
    load_checkpoint(model, path, map_location=device)
    epoch = int(getattr(model, "checkpoint_meta", {}).get("epoch", 0))
    asr = Wav2Vec2CTC.from_files(opt.asr_weights, opt.asr_config or None).to(device)
    live = LiveASR(asr, opt.l, opt.m, opt.r, opt.ring_windows, opt.tail)
    opt.aud_features = np.zeros((1, live.C, 16), dtype=np.float32)          # load_clip wants a clip's audio; LiveScene reads none of it
    scene = LiveScene(model, load_clip(opt, decode=decode), opt, device, live)
    renderer = FrameParallelRenderer(scene, rank=0, world=1, dist=None, gather_to="rank0")
    model.enc_a = None

    latency = live.warm_up_chunks / CHUNK_RATE
    if opt.wav and opt.resample:
        import io
        from .resample import Resampler, read_audio
        rate, channels, fmt, raw = read_audio(opt.wav)
        resampler = Resampler(rate, SAMPLE_RATE, fmt, channels, device=device)
        read_chunk = resampled_chunks(block_reader(io.BytesIO(raw), rate, fmt, channels), resampler)
        latency += resampler.latency
        if opt.video and not opt.audio_wav:
            opt.audio_track = cli.resampled_track(opt.wav, lambda: resampler.whole(raw), log)
    elif opt.wav:
        read_chunk = chunks_of(read_wav(opt.wav))
    else:
        stream = stdin if stdin is not None else (sys.stdin.buffer if opt.pcm == "-" else open(opt.pcm, "rb"))
        if opt.pcm_resample:
            from .resample import Resampler
            resampler = Resampler(opt.pcm_rate, SAMPLE_RATE, opt.pcm_format, opt.pcm_channels, device=device)
            read_chunk = resampled_chunks(block_reader(stream, opt.pcm_rate, opt.pcm_format, opt.pcm_channels), resampler)
            latency += resampler.latency
        else:
            read_chunk = pcm_chunks(stream)
    log(f"[INFO] live ASR: windows of {opt.l} + {opt.m} + {opt.r} chunks, expected latency = {latency:.6f}s")

    name = f"{opt.name}_ep{epoch:04d}_live"
    out_dir = os.path.join(opt.workspace, "results")
    os.makedirs(out_dir, exist_ok=True)
    if opt.video and not opt.audio_wav and getattr(opt, "audio_track", None) is None:
        opt.audio_wav = opt.wav                                         # the streamed file is laid under its own frames
    sink = cli._video_sink(opt, scene.H, scene.W, device, out_dir, name) if opt.video else None
    raw = host = None
    if opt.raw_out:
        raw = sys.stdout.buffer if opt.raw_out == "-" else open(opt.raw_out, "wb")
        host = FrameSink(scene.H, scene.W, slots=8, device=device)
    def drain(wait):
        while True:
            got = host.pop(wait=wait)
            if got is None:
                return
            raw.write(got[1].tobytes())
    frames, stamps, t0 = [], [], None
    with torch.no_grad():
        for k in schedule(live, read_chunk):
            if opt.realtime:
                t0 = time.perf_counter() if t0 is None else t0
                wait = t0 + k / opt.video_fps - time.perf_counter()
                if wait > 0:
                    time.sleep(wait)
            u8 = renderer.step(k)
            if not opt.no_npy or sink is not None or host is not None:
                u8 = u8.clone()                                         # the renderer's frame buffer is written again by the next frame
            if not opt.no_npy:
                frames.append(u8)
            if sink is not None:
                sink.push(u8)
            if host is not None:
                if host.full():
                    raw.write(host.pop(wait=True)[1].tobytes())
                host.push(u8, tag=k)
                drain(wait=False)
            stamps.append(time.perf_counter())
        renderer.finish()
    n = live.n_frames
    done = dict(opt=opt, n_frames=n, video=None, avi=None, raw_out=opt.raw_out or None, latency=latency, windows=live.windows_run,
                frame_ms=[1e3 * (b - a) for a, b in zip(stamps, stamps[1:])])
    if host is not None:
        drain(wait=True)
        raw.flush()
        if raw is not sys.stdout.buffer:
            raw.close()
    if sink is not None:
        done["avi"] = sink.finish()
        log(f"[INFO] wrote {done['avi']}: {sink.files} frames at {opt.video_fps:g} per second")
    if not opt.no_npy:
        video = torch.stack(frames).cpu().numpy() if frames else np.zeros((0, scene.H, scene.W, 3), dtype=np.uint8)
        done["video"] = os.path.join(out_dir, name + ".npy")
        np.save(done["video"], video)
        log(f"[INFO] wrote {done['video']}: {video.shape[0]} frames of {scene.H} x {scene.W}")
    log(f"[INFO] {n} frames from {live.pushed_chunks} chunks, {live.windows_run} windows through the model")
    return done


if __name__ == "__main__":
    main(sys.argv[1:])
