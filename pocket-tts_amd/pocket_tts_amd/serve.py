"""Batched serving front end: continuous batching of TTS requests over
the engine's slots, and the reference server's HTTP surface on top of it.

The reference server serializes every generation behind one mutex
(pocket-tts-cli/src/server/state.rs:69) and runs one utterance at a time per process. Here a
`BatchScheduler` owns one engine (one GPU) and a driver thread:

  1. requests wait in a queue; whenever slots are free, all waiting requests that fit are
     admitted in ONE batched admission (`ptts_slots_open`: shared text-prefill pass);
  2. every engine step advances all admitted rows together (`ptts_step`), and each row's
     1920-sample frame is handed to its request's stream as soon as it exists;
  3. a row's slot is recycled when its last frame (EOS tail or max_gen_len) has been delivered.

Works with both stepping modes of the engine (with `pipeline=True` a row's frames arrive one
step after they are computed). `MultiGpuScheduler` spreads requests over one scheduler per GPU
(replicas, no inter-GPU traffic: DESIGN.md §6) inside one process; `main(--gpus N)` instead runs
one worker process per GPU, each a whole server on one shared SO_REUSEPORT port (the weights
packed once and broadcast over RCCL at load time).

HTTP (`create_app`, FastAPI; routes of pocket-tts-cli/src/server/routes.rs:20-30):
  GET  /health             {"status": "healthy", "version": ...}
  POST /generate           JSON {text | token_ids, voice?, temperature?, eos_threshold?,
                           noise_clamp?, lsd_steps?} -> audio/wav (handlers.rs:128-213);
                           lsd_steps: this request's own Euler step count, 1 .. --max-lsd-steps
                           (requests with different counts share the batch)
  POST /stream             same body -> chunked 16-bit PCM LE (handlers.rs:215-310): the first
                           frame as soon as it exists, later frames coalesced to at most one
                           chunk per 20 ms per stream
  POST /v1/audio/speech    OpenAI body {model, input, voice?, response_format?} -> wav / pcm / flac
                           (handlers.rs:380-398)
  POST /voices/{name}      body: a mono RIFF/WAVE clip, or a safetensors file holding `audio_prompt`
                           [F x 1024]: registers (or replaces) a named voice at run time
  GET  /voices             {"voices": [names], "default": name}
Wire formats follow crates/pocket-tts/src/audio.rs:110-185 (clamp to [-1, 1], x 32767,
truncate to i16; 16-bit mono RIFF/WAVE).

Word timestamps (`--align`, off by default, with `--align-layer` and `--align-heads`; DESIGN.md
section 26): /generate and /v1/audio/speech take `timestamps: true` and then answer
`application/json`: {"audio": base64 of the bytes the route would have sent, "content_type",
"sample_rate", "words": [{"word", "start", "end"}]} (seconds of that audio; the rule is align.py).
The rows deliver one text-attention row per frame from the engine's align stage; a long-form
request's segments are offset by the samples delivered before them, pauses included. 400 for
`timestamps` on /stream, with `continuity` (under `--continuity`: send `continuity: false`), with
`token_ids`, with FLAC, for a row of more than 128 tokens (checked here, so that the engine never
refuses a batched admission over it), or without `--align`.

Per-request output format (`--wire`, the default; no reference counterpart: the reference emits
24 kHz only): /generate, /stream and /v1/audio/speech also take `sample_rate` (8000, 16000, 24000,
44100, 48000) and `encoding` (`pcm_s16le`, `ulaw`, `alaw`); one of them alone defaults the other
to 24000 / pcm_s16le, and /v1/audio/speech's `response_format` also takes `ulaw` / `alaw` (raw
G.711, 8 kHz unless `sample_rate` says otherwise). Such a row is resampled and encoded on the GPU
at the end of the Mimi decode and the scheduler hands its bytes on
untouched; requests with different formats, and with none, share a batch. /generate answers with a
WAV file of that encoding (G.711: format tag 7 / 6, 8 bits, a `fact` chunk), /stream with the raw
bytes. A request that names neither field gets today's bytes by today's code path. Unknown values,
or either field on a `--no-wire` server, get 400.

FLAC (`--flac`, on with `--wire`): `encoding: "flac"` on the three audio
routes, or `response_format: "flac"` on /v1/audio/speech, answers `audio/flac`: the row's 16-bit
samples at its `sample_rate` (and `speed`) as lossless FLAC frames, encoded on the GPU behind the
wire stage. /stream sends the 42-byte stream header and then the row's chunks untouched; /generate
and /v1/audio/speech send a complete file whose header holds the sample count. A row numbers its
samples from 0: with `long_form` or `continuity` (several rows behind one response) the engine's
frame index travels with every chunk and the frames are renumbered on the host as they are handed
over in text order, pauses being CONSTANT frames (audio.FlacJoiner), so the
response is one stream. FLAC on a server without the stage (`--no-flac`, `--no-wire`) gets 400.

    curl -s localhost:8000/v1/audio/speech -H 'content-type: application/json' \
         -d '{"input": "Hello there.", "voice": "alba", "response_format": "flac"}' -o hello.flac

Per-request speech speed (`--tempo`, on with `--wire`; the `speed` of the API /v1/audio/speech
imitates): the three audio routes also take `speed`, a factor in [0.5, 2.0]. The model has no
duration control, so the row's PCM is time-scaled on the GPU, pitch kept, ahead of the wire
conversion (a streaming WSOLA); the scheduler hands the bytes on untouched,
and requests with different speeds, and with none, share a batch. A speed with no format answers in
24000 / pcm_s16le. Unset or 1.0 changes nothing; a long-form request's every text segment carries
the speed and its pause silences keep their stated duration. A value outside the range, or a speed
on a server without the stage (`--no-tempo`, `--no-wire`), gets 400.

    curl -s localhost:8000/v1/audio/speech -H 'content-type: application/json' \
         -d '{"input": "Hello there.", "voice": "alba", "speed": 1.25}' -o fast.wav

Per-request pitch (`--pitch`, on with `--tempo`): the three audio routes also take `pitch`, in
semitones within [-12, 12]. The row's PCM is time-scaled by the WSOLA stage to 2^(pitch / 12) times
the duration its `speed` asks for and then read that many times faster by a streaming windowed-sinc
resampler on the GPU, so the pitch moves and the duration stays what `speed`
says. It is a resampling shift, the "deeper / brighter voice" control: formants move with the
fundamental. Every later stage (rate, encoding, FLAC) runs on the result unchanged. Unset or 0
changes nothing; a long-form request's every text segment carries the pitch and pauses keep their
duration. A value outside the range, a combination with `speed` for which speed / 2^(pitch / 12)
leaves [0.5, 2.0], or a pitch on a server without the stage (`--no-pitch`, `--no-tempo`, `--no-wire`),
gets 400.

    curl -s localhost:8000/v1/audio/speech -H 'content-type: application/json' \
         -d '{"input": "Hello there.", "voice": "alba", "pitch": -3}' -o deeper.wav

Per-request volume (`--volume`, on with `--wire`): the three audio routes also take `volume_db`, a
gain in dB within [-24, 24] (rounded to hundredths), and `limit`, a bool. A row with a gain, or with
`limit` true, runs through the level stage on the GPU behind speed and pitch:
the gain, then a look-ahead peak limiter (5.25 ms) that keeps every sample inside the server's
ceiling (`--limiter-ceiling-db`, -1 dBFS by default), so a positive gain never hard-clips and G.711
and FLAC streams come out at the asked level. Where no peak within 5.25 ms exceeds the ceiling the
samples are the scaled input exactly. Rate, encoding and FLAC run on the result unchanged. Unset, or
0 with `limit` unset, changes nothing; a long-form request's every text segment carries the fields
and pauses stay host-made silence. A value outside the range, or either field on a server without
the stage (`--no-volume`, `--no-wire`), gets 400.

    curl -s localhost:8000/v1/audio/speech -H 'content-type: application/json' \
         -d '{"input": "Hello there.", "voice": "alba", "volume_db": 6, "response_format": "ulaw"}' -o loud.ulaw

Loudness (`--loudness`, off by default; needs `--wire`, and `--volume` for `loudness_lufs`): a
BS.1770 meter on the GPU beside the wire stage. Every voice is calibrated once
on a fixed sentence (CALIBRATION_TEXT, CALIBRATION_SEED, the server's default parameters, no gain) as
an ordinary request through the scheduler: when it is registered (`--voice`, `POST /voices/NAME`), or
on first use for a per-request clip; `GET /voices/NAME` answers `{"name", "frames",
"loudness_lufs"}`. `loudness_lufs` on the three audio routes, a target in [-40, -5], gives the rows
the constant gain round(100 (target - voice loudness)) / 100 dB within [-24, 24], limiter on, reported
as `X-Gain-dB`; it excludes `volume_db`. `loudness: true` on /generate and /v1/audio/speech meters
the response (`X-Loudness-LUFS`, `none` if unmeasurable; a `loudness_lufs` key with `timestamps`),
pooled over a long-form request's segments; /stream answers 400 to it. A target out of range, a
server without the stages, or a voice whose calibration is unmeasurable gets 400.

    curl -s localhost:8000/v1/audio/speech -H 'content-type: application/json' \
         -d '{"input": "Hello there.", "voice": "alba", "loudness_lufs": -16}' -o level.wav

Long-form requests (`long_form` in the three audio routes' bodies; `--long-form` sets the default,
off): the text is cut as the reference's routes cut it (generate_stream_long, handlers.rs:165,260:
pause markers and natural pauses become silence, each piece is cut into sentence chunks of at most
50 tokens) and the chunks run as rows of the batch, at most `--segment-rows` of one request at a
time, delivered in text order behind one Request-like RequestGroup. A
/stream client that disconnects cancels its request: its rows stop without a drain of the engine
(Request.cancel, Engine.cancel_slots).

Per-request voices (pocket-tts-cli/src/voice.rs:67-222): the `voice` field is first a registered
name; else base64 WAV audio, as a `data:audio/...;base64,` URL or as raw base64 (voice.rs:172-189:
longer than 100 characters, base64 alphabet only); else the request is refused (400). The clip is
cloned as a voice job (Engine.voice_job) started by the scheduler thread between two engine calls
and admitted in the same pass, so cloning never drains the pipeline of the streams being generated
(what a clone and a cache eviction still cost them: DESIGN.md section 16). Each
engine keeps its clones in an LRU cache (`--voice-cache N`, the reference's VoiceCache,
handlers.rs:99-126) keyed by the blake2b hash of the WAV bytes and the clone settings; requests
that bring the same new clip share one job. Clips must be mono and at most `--max-voice-seconds`.

Deliberate divergence from the reference: file paths and `hf://` specs in the `voice` field are NOT
accepted from the network (the reference resolves both, voice.rs:93-102): a request must not make
the server read its own file system or fetch from outside. Such specs get the 400 of an unknown
voice. The reference's multipart /tts route is not implemented.
"""

from __future__ import annotations

import base64
import binascii
import hashlib
import math
import os
import queue
import re
import struct
import threading
import time
from collections import OrderedDict, deque
from dataclasses import dataclass, field, replace
from typing import Callable, Iterator, Sequence

import numpy as np

from ._lib import ALIGN_TOKENS, FRAME, LDIM, SAMPLE_RATE, WIRE_RATES
from .audio import (LoudnessMeter, loudness_gain_cdb, loudness_integrated,  # noqa: F401
                    ENCODINGS, FlacJoiner, flac_stream_header, level_cdb, level_limit, pcm_i16_le_bytes, wav_bytes,  # noqa: F401 (re-exported wire formats)
                    wire_bytes, wire_samples)
from .engine import GenerationParams, OutputOptions, Voice
from .text import (CALIBRATION_SEED, CALIBRATION_TEXT, estimate_frames_after_eos, long_form_segments, max_gen_len, prepare_text_prompt, segment_request,
                   silence_samples)

VERSION = "0.1.0"


# wire formats (audio.rs:110-185) live in .audio: pcm_i16_le_bytes, wav_bytes


class FrameChannel:
    """One producer (the scheduler thread), one consumer: the queue.Queue calls a Request's
    consumers use (put / get / get_nowait / empty), without a lock and condition round trip per
    frame. A deque append is atomic under the GIL, so put() is one append and, only while a
    consumer is blocked in get(), one notify (the scheduler delivers 32 frames per ~0.6-ms step:
    a locked Queue.put per frame cost it a large share of the step)."""

    def __init__(self):
        self._d: deque = deque()
        self._cv = threading.Condition(threading.Lock())
        self._waiting = False

    def put(self, item):
        self._d.append(item)
        if self._waiting:  # the consumer set this before it checked the deque: it sees either
            with self._cv:  # the appended item or this notify
                self._cv.notify()

    def get_nowait(self):
        try:
            return self._d.popleft()
        except IndexError:
            raise queue.Empty from None

    def empty(self) -> bool:
        return not self._d

    def get(self, timeout: float | None = None):
        try:
            return self._d.popleft()
        except IndexError:
            pass
        deadline = None if timeout is None else time.monotonic() + timeout
        with self._cv:
            self._waiting = True
            try:
                while not self._d:
                    rem = None if deadline is None else deadline - time.monotonic()
                    if rem is not None and rem <= 0:
                        raise queue.Empty
                    self._cv.wait(rem)
                return self._d.popleft()
            finally:
                self._waiting = False


# ---------------------------------------------------------------------------------------------
@dataclass
class VoiceClip:
    """A voice still to be cloned, on whichever engine its request is routed to: a mono clip in its
    wire format (int16 or float32) with the clone settings, or a precomputed audio_prompt. `key`
    identifies it in that engine's VoiceCache; n_frames is computed on the host (as the engine does)."""

    key: bytes
    n_frames: int
    samples: np.ndarray | None = None
    sample_rate: int = SAMPLE_RATE
    chunk_frames: int = 0
    resampler: str = "poly"
    prompt: np.ndarray | None = None

    def start(self, engine) -> Voice:
        """Start the clone as a voice job; the returned voice can be admitted at once."""
        if self.prompt is not None:
            return engine.voice_job_prompt(self.prompt)
        return engine.voice_job(self.samples, self.sample_rate, self.chunk_frames, self.resampler)


def clip_frames(n_samples: int, sample_rate: int, resampler: str = "poly") -> int:
    """Conditioning frames of a clip: its length at 24 kHz (the engine's host-side rule) in whole
    1920-sample frames."""
    if sample_rate == SAMPLE_RATE:
        n = n_samples
    elif resampler == "rubato":
        from ._lib import lib
        from .engine import resampler_code

        n = lib().ptts_resample_len_ex(int(n_samples), int(sample_rate), SAMPLE_RATE, resampler_code(resampler))
    else:
        g = math.gcd(int(sample_rate), SAMPLE_RATE)
        up, down = SAMPLE_RATE // g, int(sample_rate) // g
        n = (n_samples * up + down - 1) // down
    return (n + FRAME - 1) // FRAME


class VoiceCache:
    """LRU of the voices an engine cloned for its requests (the reference's VoiceCache,
    handlers.rs:99-126), used by the scheduler thread only. A voice enters when its job is
    started, so later requests with the same clip share that job. trim() drops the least recently
    used entries past the capacity: only the cache's reference goes, a voice that slots still read
    lives on until the last of them lets go (ptts_voice_destroy)."""

    def __init__(self, capacity: int = 64):
        self.capacity = max(int(capacity), 0)
        self._d: OrderedDict[bytes, Voice] = OrderedDict()
        self.jobs = 0  # clones started
        self.hits = 0

    def __len__(self):
        return len(self._d)

    def keys(self):
        return list(self._d)

    def get_or_start(self, clip: VoiceClip, engine) -> Voice:
        v = self._d.get(clip.key)
        if v is not None:
            self._d.move_to_end(clip.key)
            self.hits += 1
            return v
        v = clip.start(engine)
        self.jobs += 1
        self._d[clip.key] = v
        return v

    def trim(self, keep: int | None = None):
        while len(self._d) > (self.capacity if keep is None else keep):
            self._d.popitem(last=False)[1].close()


class _Call:
    def __init__(self, fn):
        self.fn, self.done, self.result, self.error = fn, threading.Event(), None, None

    def run(self):
        try:
            self.result = self.fn()
        except BaseException as e:  # handed to the caller
            self.error = e
        self.done.set()


def row_output(params) -> OutputOptions:
    """The output options of a row's params (a foreign params object that has none: the defaults)."""
    return params.output() if hasattr(params, "output") else OutputOptions()


def item_samples(item, wire) -> int:
    """Samples of one delivered item: wire bytes of the format `wire` (rate, encoding), a FLAC chunk
    with its frame index (a segment of a FLAC group), or f32 frames."""
    if isinstance(item, tuple):
        return sum(int(bs) for _, bs in item[1])
    if isinstance(item, (bytes, bytearray)):
        return len(item) // (1 if wire is not None and wire[1] in ("ulaw", "alaw") else 2)
    return int(np.size(item))


class _Consumer:
    """The consumer side of a Request or a RequestGroup: items from `out` until the end marker."""

    def loudness(self) -> float | None:
        """Integrated loudness in LUFS of a finished metered request (its audio consumed), the gating
        blocks of all its rows pooled and gated once; None: unmeasurable, or not metered."""
        rows = [it for it in getattr(self, "items", [self]) if isinstance(it, Request) and it.loud_rows is not None]
        energy = [np.concatenate(it.loud_rows) if it.loud_rows else np.zeros(0, np.float64) for it in rows]
        return loudness_integrated(energy) if energy else None

    def stream(self, timeout: float | None = None) -> Iterator[np.ndarray]:
        """Frames [1920] float32 as they are produced; raises the driver's error if any."""
        while True:
            item = self.out.get(timeout=timeout)
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def stream_batches(self, timeout: float | None = None) -> Iterator[np.ndarray]:
        """Like stream(), but each item is every frame available at that moment, concatenated
        (at least one): a client that falls behind the engine gets one HTTP chunk per backlog
        instead of one per frame, so per-chunk server overhead cannot throttle the stream."""
        done = False
        while not done:
            frames = [self.out.get(timeout=timeout)]
            while True:
                try:
                    frames.append(self.out.get_nowait())
                except queue.Empty:
                    break
            batch = []
            for item in frames:
                if item is None:
                    done = True
                    break
                if isinstance(item, BaseException):
                    raise item
                batch.append(item)
            if batch:
                yield batch[0] if len(batch) == 1 else np.concatenate(batch)

    def audio(self, timeout: float | None = None) -> np.ndarray:
        frames = list(self.stream(timeout))
        return np.concatenate(frames) if frames else np.zeros(0, np.float32)

    def wire_audio(self, timeout: float | None = None) -> bytes:
        """A wire request's whole output: its chunks joined, untouched."""
        return b"".join(self.stream(timeout))

    def cancel(self):
        """Stop the request (its client went away): the scheduler thread drops what of it still
        waits, stops its rows at its next pass without draining the engine (Engine.cancel_slots)
        and ends the stream. Callable from any thread; a finished request is left alone."""
        s = self.sched
        if s is not None:
            s._cancel(self)


@dataclass
class Request(_Consumer):
    ids: np.ndarray
    voice: Voice | None
    params: GenerationParams
    clip: VoiceClip | None = None  # voice still to be cloned (resolved by the scheduler thread at admission)
    out: FrameChannel = field(default_factory=FrameChannel)  # np.ndarray frames, then None
    slot: int = -1
    frames: int = 0
    waker: Callable[[], None] | None = None  # set by an async consumer (HTTP /stream)
    times: dict = field(default_factory=dict)  # submit / admit / first / last (time.time())
    # first-frame preview: 1 = the preview was delivered as frame 0 and the regular frame 0 is still
    # to come (it is dropped), 2 = that frame came
    preview: int = 0
    start_step: int = 0  # the scheduler's step that starts the row (trace)

    # (sample_rate, encoding name) of a request with a wire format: its items are bytes the engine
    # converted (Engine.fetch_wire), not float32 frames; None: today's float32 frames
    wire: tuple[int, str] | None = None
    speed: int = 0         # permille of a request with a speed (its wire bytes are time-scaled); 0: none
    pitch: int = 0         # cents of a request with a pitch (its wire bytes are shifted); 0: none
    level: tuple = (0, 0)  # (gain in hundredths of a dB, limit) of a request in the level stage; (0, 0): none
    sched: object = None   # the scheduler that holds the request (cancel())
    group: object = None   # the RequestGroup this request is a text segment of
    ended: bool = False    # the end marker was put
    # continuity: a segment of a continuity group keeps the latents of its
    # frames (lat; None: not kept), and one that follows another text segment with no pause in
    # between names it (pred): it is admitted on pred's slot behind pred's ids and latents (own: the
    # segment's own ids, which `ids` then follows pred's in)
    lat: list | None = None
    pred: object = None
    own: np.ndarray | None = None
    # timestamps: the alignment row of every frame of a row in the align stage
    # (None: not in it), and the samples handed over so far at the rate they are delivered at
    align_rows: list | None = None
    units: int = 0
    # loudness: the sub-block energies of every frame of a metered row (None:
    # not metered), and the gain in dB a `loudness_lufs` request was given (None: none)
    loud_rows: list | None = None
    gain_db: float | None = None

    def __post_init__(self):
        if getattr(self.params, "align", False):
            self.align_rows = []
        if getattr(self.params, "loudness", False):
            self.loud_rows = []
        out = row_output(self.params)
        self.wire = out.wire or self.wire
        _, _, self.speed, self.pitch, *lv = out.codes()
        self.level = tuple(lv)

    def put(self, item):
        """Driver side: hand over a frame (np.ndarray), the end marker (None) or an error."""
        if item is None:
            self.ended = True
        elif not isinstance(item, BaseException):
            self.units += item_samples(item, self.wire)
        g = self.group
        if g is not None:  # a segment of a long-form request: its group puts the items in text order
            g.deliver(self, item)
            return
        self.out.put(item)
        w = self.waker
        if w is not None:
            w()

    def _end(self):
        if not self.ended:
            self.put(None)


class RequestGroup(_Consumer):
    """A long-form request: the ordered segments of one text, pauses
    (ready-made silence items) and text segments (Requests the scheduler runs as rows like any
    other), behind the consumer surface of one Request. A segment's items are held back until every
    earlier segment and pause has been handed over; at most `rows` text segments are waiting or
    active at once, the next one joining the tail of the scheduler's queue when one finishes.
    deliver() runs on the scheduler thread only.
    A FLAC group (section 21.5): its segments' items are (chunk, frame index), its pauses sample
    counts, and both pass through `joiner` as they are handed over, which numbers them as one stream;
    joiner.total is the response's sample count once it has ended."""

    def __init__(self, sched, items, rows: int, wire, continuity: bool = False):
        self.sched, self.items, self.rows, self.wire = sched, items, max(1, int(rows)), wire
        self.continuity = bool(continuity)  # one segment at a time, each continuing the one before it
        self.joiner = FlacJoiner(wire[0]) if wire is not None and wire[1] == "flac" else None
        self.out = FrameChannel()
        self.waker: Callable[[], None] | None = None
        self.times: dict = {"submit": time.time()}
        self.segments = [it for it in items if isinstance(it, Request)]
        self.pending: deque[Request] = deque(self.segments)  # not yet handed to the scheduler
        self.buf = {id(r): [] for r in self.segments}
        self.head = 0
        self.frames = 0
        self.ended = False
        for r in self.segments:
            r.group = self

    def _emit(self, item):
        if item is not None and "first" not in self.times:
            self.times["first"] = time.time()
        self.out.put(item)
        w = self.waker
        if w is not None:
            w()

    def _end(self):
        """The end marker, once; nothing of the group is handed over after it."""
        if not self.ended:
            self.ended = True
            self.pending.clear()
            self.times["last"] = time.time()
            self._emit(None)

    def _pump(self):
        while not self.ended and self.head < len(self.items):
            it = self.items[self.head]
            if isinstance(it, Request):
                buf = self.buf[id(it)]
                for x in buf:
                    self.frames += 1
                    if self.joiner is not None:
                        x = self.joiner.chunk(*x)
                        if not x:
                            continue
                    self._emit(x)
                buf.clear()
                if not it.ended:
                    return
                if self.joiner is not None:
                    self.joiner.end_segment()
            elif self.joiner is not None:
                x = self.joiner.pause(it)
                if x:
                    self._emit(x)
            else:
                self._emit(it)
            self.head += 1
        self._end()

    def deliver(self, seg: Request, item):
        if self.ended:
            return
        if isinstance(item, BaseException):  # a segment failed: the group fails once, the rest is torn down
            self._emit(item)
            self._end()
            self.sched._cancel(self)
            return
        if item is not None:
            self.buf[id(seg)].append(item)
        if self.items[self.head] is seg:
            self._pump()


class BatchScheduler:
    """Continuous batching over one engine's slots (one GPU).

    On a pipelined engine a new row's first frame would trail its first step by the pipeline's
    frame lag (three calls with frame-pair passes). With `preview_rows` > 0 the engine also decodes
    each new row's first frame on its own right after that step (ptts_preview_enable); the
    scheduler delivers that preview as the request's frame 0 and drops the regular frame 0 when it
    comes (the two agree within float rounding: the regular pass decodes it from the same fresh
    state), or, if the regular frame comes first, drops the preview."""

    def __init__(self, engine, max_rows: int | None = None, preview_rows: int = 8, voice_cache: int = 64,
                 segment_rows: int = 4):
        """segment_rows: how many text segments of one long-form request (submit_group) may be
        waiting or active at once (a policy knob: more rows finish a long text sooner and leave
        fewer to other requests)."""
        self.engine = engine
        self.voices = VoiceCache(voice_cache)  # per-request clones of this engine
        self.calls: deque[_Call] = deque()     # engine work handed to the scheduler thread (call())
        self.retired: list = []                # replaced voices, closed once no queued request holds them
        self.max_rows = min(max_rows or engine.max_slots, engine.max_slots)
        self.preview = bool(preview_rows) and getattr(engine, "pipeline", False) and hasattr(engine, "enable_preview")
        if self.preview:
            engine.enable_preview(preview_rows)
        self.previews = 0  # first frames delivered from a preview
        self.poll_s = 50e-6
        self.shallow = getattr(engine, "pipeline", False) and hasattr(engine, "front_done")
        self.segment_rows = max(1, min(int(segment_rows), self.max_rows))
        self.waiting: deque[Request] = deque()
        self.active: dict[int, Request] = {}
        self.cancels: deque = deque()  # requests / groups to stop at the next pass (cancel())
        # continuity successors that were handed their predecessor's slot (already in `active`): they
        # join the next batched admission
        self.handoff: list[Request] = []
        # calls by which a fetched frame trails the step that computed it
        self.lag = int(bool(getattr(engine, "pipeline", False)))  # (an engine without frame_lag: one call if pipelined)
        if hasattr(engine, "frame_lag"):
            self.lag = engine.frame_lag()[0]
        # slots freed by a cancel on an engine without cancel_slots: the old row's frames are told
        # from the next request's by the step that computed them (Request.start_step)
        self.stale: set[int] = set()
        self.cv = threading.Condition()
        self.running = True
        self.steps = 0
        self.row_frames = 0  # frames delivered (valid rows summed over steps)
        self.trace = bool(os.environ.get("PTTS_SERVE_TRACE"))
        # called (under self.cv) with the new load whenever it changes: the multi-process server
        # publishes it on its LoadBoard for the overflow redirect
        self.on_load: Callable[[int], None] | None = None
        self.thread = threading.Thread(target=self._loop, name="ptts-scheduler", daemon=True)
        self.thread.start()

    # -- client side
    def submit(self, ids, voice: Voice | VoiceClip, params: GenerationParams) -> Request:
        """voice: a Voice of this engine, or a VoiceClip: cloned (or found in the cache) by the
        scheduler thread right before the request's admission, in the same pass."""
        req = self._new_request(ids, voice, params)
        with self.cv:
            if not self.running:
                raise RuntimeError("scheduler stopped")
            self.waiting.append(req)
            if self.on_load is not None:
                self.on_load(len(self.active) + len(self.waiting))
            self.cv.notify()
        return req

    def _new_request(self, ids, voice, params) -> Request:
        req = Request(np.asarray(ids, np.int32).reshape(-1), voice, params, sched=self)
        if isinstance(voice, VoiceClip):
            req.voice, req.clip = None, voice
        req.times["submit"] = time.time()
        if voice.n_frames + req.ids.size + params.max_frames > self.engine.max_ctx:
            raise ValueError("voice + text + max_frames exceeds the engine's max_ctx")
        return req

    def submit_group(self, segments, voice: Voice | VoiceClip, wire: tuple[int, str] | None = None,
                     segment_rows: int | None = None, continuity: bool = False) -> RequestGroup:
        """A long-form request: segments in text order, ("text", ids, params) | ("pause", ms). Every
        text segment is an utterance of its own (the max_ctx rule of submit() applies to each); a
        pause becomes silence, in the group's wire format (`wire`: (rate, encoding)) if it has one.
        continuity: the group runs one text segment at a time, and a segment
        that follows another with no pause in between takes over its slot when its last frame is
        delivered, admitted with the two segments' ids, the predecessor's delivered latents as a
        teacher-forced prefix and keep_codec (where that exceeds max_ctx: as a plain segment). A
        pause starts a new chain."""
        items = []
        for seg in segments:
            if seg[0] == "text":
                items.append(self._new_request(seg[1], voice, seg[2]))
                if continuity:
                    items[-1].lat, items[-1].own = [], items[-1].ids
                    if len(items) > 1 and isinstance(items[-2], Request):
                        items[-1].pred = items[-2]
            elif wire is not None and wire[1] == "flac":
                items.append(silence_samples(seg[1], wire[0]))  # encoded at its place (RequestGroup._pump)
            elif wire is not None:
                items.append(wire_bytes(np.zeros(silence_samples(seg[1], wire[0]), np.float32), wire[1]))
            else:
                items.append(np.zeros(silence_samples(seg[1], SAMPLE_RATE), np.float32))
        rows = self.segment_rows if segment_rows is None else max(1, min(int(segment_rows), self.max_rows))
        g = RequestGroup(self, items, 1 if continuity else rows, wire, continuity)
        with self.cv:
            if not self.running:
                raise RuntimeError("scheduler stopped")
            g._pump()  # leading pauses (and a text of pauses only) need no row
            for _ in range(min(g.rows, len(g.pending))):
                self.waiting.append(g.pending.popleft())
            if self.on_load is not None:
                self.on_load(len(self.active) + len(self.waiting))
            self.cv.notify()
        return g

    def load(self) -> int:
        with self.cv:
            return len(self.active) + len(self.waiting)

    def _cancel(self, target):
        with self.cv:
            if self.running:
                self.cancels.append(target)
                self.cv.notify()

    def _reap(self) -> list[int]:
        """(under self.cv, ahead of _take) drop what the cancelled requests and groups still have
        waiting, free their rows' slots (admissible in this pass) and end their streams; returns
        the slots whose rows the engine is to stop."""
        slots = []
        while self.cancels:
            t = self.cancels.popleft()
            mine = {id(r) for r in (t.segments if isinstance(t, RequestGroup) else [t])}
            if any(id(r) in mine for r in self.waiting):
                self.waiting = deque(r for r in self.waiting if id(r) not in mine)
            self.handoff = [r for r in self.handoff if id(r) not in mine]
            for slot, r in list(self.active.items()):
                if id(r) in mine:
                    del self.active[slot]
                    slots.append(slot)
            t._end()
        if self.on_load is not None:
            self.on_load(len(self.active) + len(self.waiting))
        return slots

    def call(self, fn):
        """Run fn() on the scheduler thread between two engine calls (engine calls stay on one
        thread) and return its result; its exception is raised here."""
        c = _Call(fn)
        with self.cv:
            if not self.running:
                raise RuntimeError("scheduler stopped")
            self.calls.append(c)
            self.cv.notify()
        c.done.wait()
        if c.error is not None:
            raise c.error
        return c.result

    def retire(self, voice):
        """Close a voice of this engine that the caller no longer hands out, once no waiting
        request holds it (an admitted row keeps its voice alive by itself, ptts_voice_destroy). A
        caller that resolves a name and submits under one lock, and swaps the name under the same
        lock before retiring, cannot queue a request with a closed voice."""
        try:
            self.call(lambda: (self.retired.append(voice), self._close_retired()))
        except RuntimeError:  # scheduler stopped: nothing is queued any more
            voice.close()

    def _close_retired(self):
        """(scheduler thread, after the pass's admission)"""
        if not self.retired:
            return
        with self.cv:
            held = {id(r.voice) for r in self.waiting}
        keep = [v for v in self.retired if id(v) in held]
        for v in self.retired:
            if id(v) not in held:
                v.close()
        self.retired = keep

    def close(self):
        with self.cv:
            self.running = False
            self.cv.notify()
        self.thread.join()
        self.voices.trim(0)
        for v in self.retired:
            v.close()
        self.retired = []

    # -- driver thread
    def _continue(self, req: Request, nxt: Request, slot: int) -> bool:
        """(under self.cv) make `nxt` the continuation of `req`, whose last frame was just delivered
        from `slot`: the two segments' ids, req's delivered latents (its EOS tail included) as the
        prefix, keep_codec, on the same slot, in the next batched admission. False (nxt untouched: a
        plain segment) where the engine's capacity rule would refuse it."""
        pre = np.array(req.lat, np.float32).reshape(-1, LDIM)
        voice = nxt.voice if nxt.voice is not None else nxt.clip
        if voice.n_frames + req.own.size + nxt.own.size + pre.shape[0] + nxt.params.max_frames > self.engine.max_ctx:
            return False
        nxt.ids = np.concatenate([req.own, nxt.own])
        nxt.params = replace(nxt.params, prefix_latents=pre, keep_codec=True)
        nxt.slot = slot
        self.active[slot] = nxt
        self.handoff.append(nxt)
        return True

    def _take(self) -> list[Request]:
        """(under self.cv) waiting requests that fit the free slots, slots assigned and reserved"""
        free = [s for s in range(self.max_rows) if s not in self.active]
        batch, self.handoff = self.handoff, []
        while self.waiting and free:
            req = self.waiting.popleft()
            req.slot = free.pop(0)
            self.active[req.slot] = req
            batch.append(req)
        return batch

    def _refuse(self, batch: list[Request], reqs: list[Request], err: BaseException):
        """Fail `reqs` of the taken batch with err and free their slots."""
        with self.cv:
            for r in reqs:
                batch.remove(r)
                del self.active[r.slot]
            if self.on_load is not None:
                self.on_load(len(self.active) + len(self.waiting))
        for r in reqs:
            r.put(err)
            r.put(None)

    def _admit(self, batch: list[Request]):
        """(outside self.cv: submit() runs on the HTTP event loop and must never wait for an
        admission's engine call) one batched admission of the taken requests"""
        for r in list(batch):  # per-request voices: found in the cache, or their job started here
            if r.voice is None:
                try:
                    r.voice = self.voices.get_or_start(r.clip, self.engine)
                except Exception as e:  # the engine refused the clip: this request fails, the rest go on
                    self._refuse(batch, [r], e)
            elif getattr(r.voice, "handle", True) is None:  # closed under the request: it alone fails
                self._refuse(batch, [r], RuntimeError("the request's voice was closed before its admission"))
        if not batch:
            return
        try:
            self.engine.open_many([r.slot for r in batch], [r.voice for r in batch], [r.ids for r in batch],
                                  [r.params for r in batch])
        except Exception as e:
            # an argument the engine refused (PTTS_ERR_INVALID: checked before anything is enqueued)
            # fails the admission's own requests and the streams being generated go on; any other
            # failure (HIP, state) still stops the scheduler
            if getattr(e, "code", 1) != 1:
                raise
            self._refuse(batch, list(batch), e)
            return
        self.voices.trim()  # after the admission: the slots hold their voices now
        now = time.time()
        # the rows start at the step issued admit_delay calls after the next one (ptts_frame_lag)
        delay = self.engine.frame_lag()[1] if hasattr(self.engine, "frame_lag") else 0
        for r in batch:
            r.times["admit"] = now
            r.start_step = self.steps + delay

    def _deliver_previews(self):
        if not self.preview:
            return
        for slot, pcm in self.engine.fetch_previews():
            req = self.active.get(slot)
            if req is None or req.frames or req.preview:  # the regular frame 0 came first
                continue
            fmt = req.wire
            if fmt is not None:
                # a resampled row's first chunk is shorter than its preview's frame (the filter's
                # delay): it waits for its regular first chunk; a 24 kHz row's preview is encoded here
                # a speed or pitch row's first chunk is not its first frame either
                # a FLAC row's frames are written by the engine alone
                # a level row's first chunk trails its first frame by the look-ahead
                if fmt[0] != SAMPLE_RATE or req.speed or req.pitch or fmt[1] == "flac" or req.level != (0, 0):
                    continue
                pcm = wire_bytes(pcm, fmt[1])
            req.preview = 1
            req.frames = 1
            self.row_frames += 1
            self.previews += 1
            req.times["first"] = time.time()
            req.put(pcm)

    def _deliver(self, res, rows, wire=None, fstep: int = 0, align=None, findex=None, loud=None) -> list[int]:
        """wire: the call's Engine.fetch_wire chunks (a call with wire rows): those rows get their
        bytes untouched; numpy is called for rows without a format only (by their consumers).
        findex: the call's Engine.fetch_flac_index (a call with a FLAC segment of a group): such a
        row's item is (chunk, index), which its group renumbers.
        fstep: the step that computed the call's frame."""
        done = []
        for slot, req in list(self.active.items()):
            if slot < rows and res.valid[slot]:
                if self.stale and slot in self.stale:
                    if fstep < req.start_step:  # still the cancelled row's frame
                        continue
                    self.stale.discard(slot)
                if req.lat is not None:  # a continuity segment: what its successor is forced through
                    req.lat.append(np.array(res.latents[slot], np.float32))
                if req.align_rows is not None:  # (frame 0's row comes with the regular frame, preview or not)
                    req.align_rows.append(np.array(align[slot], np.float32))
                if req.loud_rows is not None:  # (likewise: the meter saw the regular frame)
                    req.loud_rows.append(np.array(loud[slot], np.float64))
                if req.preview == 1:  # frame 0, already delivered from the preview
                    req.preview = 2
                else:
                    req.frames += 1
                    self.row_frames += 1
                    if req.frames == 1:
                        req.times["first"] = time.time()
                    # a view: fetch() returns fresh arrays every step
                    if req.wire is None:
                        req.put(res.pcm[slot])
                    elif findex is not None and req.group is not None and req.wire[1] == "flac":
                        req.put((wire[slot], findex[slot]))
                    else:
                        req.put(wire[slot])
                if res.last[slot]:
                    req.times["last"] = time.time()
                    if self.trace:
                        t = req.times
                        t0 = t.get("route", t["submit"])
                        ts = t.get("start", t["submit"])
                        print(f"ptts-serve slot {slot} route_to_submit_ms {1e3 * (t['submit'] - t0):.1f} "
                              f"start_ms {1e3 * (ts - t['submit']):.2f} "
                              f"first_after_start_ms {1e3 * (t['first'] - ts):.2f} "
                              f"first_to_chunk0_ms {1e3 * (t.get('chunk0', t['first']) - t['first']):.1f} "
                              f"frames {req.frames} admit_wait_ms "
                              f"{1e3 * (t['admit'] - t['submit']):.1f} first_ms {1e3 * (t['first'] - t['submit']):.1f} "
                              f"last_ms {1e3 * (t['last'] - t['submit']):.1f} steps {self.steps}", flush=True)
                    req.put(None)
                    done.append(slot)
        return done

    def _loop(self):
        # One call in flight: call k+1 is issued (step_async) before the frames of call k are
        # fetched and handed out, so the GPU always has the next step queued while this thread
        # waits for the GIL (the HTTP event loop shares it) and delivers frames. A finished row is
        # released when its last frame is delivered (later calls compute it as inactive:
        # frame_valid = 0).
        issued: deque[int] = deque()  # rows of the calls issued and not fetched yet (<= 2)
        calls: list[_Call] = []       # this pass's share of self.calls
        try:
            while True:
                with self.cv:
                    while (self.running and not self.waiting and not self.active and not issued and not self.calls
                           and not self.cancels):
                        self.cv.wait()
                    if not self.running:
                        break
                    calls = list(self.calls)
                    self.calls.clear()
                    stop = self._reap() if self.cancels else []
                    batch = self._take()
                    rows = max(self.active) + 1 if self.active else 0
                # A pipelined engine lets the host run calls ahead of the GPU (the fetch below waits
                # for a frame several calls old), and an admission queues behind every FlowLM step
                # already issued: keep one step queued behind the running one, no more, so a new
                # row's prefill and first step wait for one step at most (first-chunk latency; the
                # GPU still always has the next step queued)
                if self.shallow and issued:
                    self.engine.front_done(1, wait=True)
                if stop:  # before the admission: a freed slot may be admitted again in this pass
                    if hasattr(self.engine, "cancel_slots"):
                        self.engine.cancel_slots(sorted(stop))  # no drain: the other rows keep stepping
                    else:
                        self.stale.update(stop)  # the rows run out; their frames are discarded
                if batch:
                    self._admit(batch)
                    rows = max(self.active) + 1 if self.active else 0  # a refused request freed its slot
                # after the admission: every request this pass took holds its voice in the engine
                # by now, so a retired voice is kept for the requests still waiting only
                for c in calls:
                    c.run()
                calls = []
                self._close_retired()
                if rows:
                    self.engine.step_async(rows)
                    issued.append(rows)
                    if self.trace:
                        now = time.time()
                        for r in self.active.values():
                            if r.start_step == self.steps:
                                r.times["start"] = now
                    self.steps += 1
                self._deliver_previews()
                if len(issued) == 2 or (issued and not rows):
                    cb = len(issued) - 1
                    # while a stream waits for its first frame, poll the call's frame and the
                    # previews (~50 us apart) instead of blocking in fetch(): a preview completes
                    # while the call's back pass still runs, and is handed out as soon as it does
                    if self.preview and any(r.frames == 0 for r in self.active.values()):
                        while not self.engine.fetch_ready(cb):
                            self._deliver_previews()
                            time.sleep(self.poll_s)
                    res = self.engine.fetch(issued[0], calls_back=cb)
                    wire = None
                    if any(r.wire is not None for r in self.active.values()):
                        wire = self.engine.fetch_wire(issued[0], calls_back=cb)
                    findex = None  # the segments of a FLAC group are renumbered: their chunks need the frame index
                    if any(r.group is not None and r.wire is not None and r.wire[1] == "flac" for r in self.active.values()):
                        findex = self.engine.fetch_flac_index(issued[0], calls_back=cb)
                    arows = None
                    if any(r.align_rows is not None for r in self.active.values()):
                        arows = self.engine.fetch_align(issued[0], calls_back=cb)
                    lrows = None
                    if any(r.loud_rows is not None for r in self.active.values()):
                        lrows = self.engine.fetch_loud(issued[0], calls_back=cb)
                    self._deliver_previews()  # those that completed while fetch() waited: ahead of it
                    fstep = self.steps - len(issued) - self.lag
                    done = self._deliver(res, issued.popleft(), wire, fstep, arows, findex, lrows)
                    if done:
                        with self.cv:
                            for slot in done:
                                req = self.active.pop(slot)
                                g = req.group
                                # a long-form request's next segment joins the tail of the queue
                                if g is not None and g.pending and not g.ended:
                                    nxt = g.pending.popleft()
                                    if nxt.pred is req and self._continue(req, nxt, slot):
                                        continue  # the slot went straight to the successor
                                    self.waiting.append(nxt)
                            if self.on_load is not None:
                                self.on_load(len(self.active) + len(self.waiting))
        except BaseException as e:  # deliver the failure to every waiting client
            with self.cv:
                self.running = False
                for req in list(self.active.values()) + list(self.waiting):
                    req.put(e)
                    req.put(None)
                self.active.clear()
                self.waiting.clear()
        finally:
            with self.cv:
                self.running = False
                for req in list(self.active.values()) + list(self.waiting):
                    if req.group is not None:
                        req.group._end()
                    else:
                        req.put(None)
                for c in list(calls) + list(self.calls):  # also those this pass took and never ran
                    if not c.done.is_set():
                        c.error = RuntimeError("scheduler stopped")
                        c.done.set()
                self.calls.clear()


class MultiGpuScheduler:
    """Replicas: one BatchScheduler per GPU engine; a request goes to the least loaded one."""

    def __init__(self, schedulers: Sequence[BatchScheduler]):
        self.schedulers = list(schedulers)

    def submit(self, ids, voices: Sequence[Voice] | VoiceClip, params: GenerationParams) -> Request:
        """voices: one Voice per GPU, or a VoiceClip: cloned on the engine the request is routed to
        (each engine has its own cache)."""
        i = min(range(len(self.schedulers)), key=lambda k: self.schedulers[k].load())
        return self.schedulers[i].submit(ids, voices if isinstance(voices, VoiceClip) else voices[i], params)

    def submit_group(self, segments, voices: Sequence[Voice] | VoiceClip, wire=None,
                     continuity: bool = False) -> RequestGroup:
        i = min(range(len(self.schedulers)), key=lambda k: self.schedulers[k].load())
        v = voices if isinstance(voices, VoiceClip) else voices[i]
        if continuity:
            return self.schedulers[i].submit_group(segments, v, wire, continuity=True)
        return self.schedulers[i].submit_group(segments, v, wire)

    def close(self):
        for s in self.schedulers:
            s.close()


class LoadBoard:
    """Least-loaded dispatch for the multi-process server (BASELINE configs[3]: 256 streams over 8
    GPUs). The kernel spreads connections over the workers of the shared SO_REUSEPORT port by a hash,
    blind to load, and a keep-alive connection stays on its worker; so each worker publishes its
    load (requests active + waiting) and the port of a private listener in one small file under
    /dev/shm that every worker of the server maps, and a worker with no free slot answers a request
    on the shared port with 307 (method and body kept) to the private port of the least-loaded peer
    that has one. Requests on a private port are always served (a request is redirected at most
    once). One int64 quadruple per rank: (load, private port, pid, process start time). Each worker
    resets its own entry when it maps the board, and a peer is a target only while a process with
    that pid AND that start time (/proc/<pid>/stat field 22) exists, so an entry left by a crashed
    worker, or by an earlier server on the same port, is not redirected to even after the pid has
    been reused by another process."""

    FIELDS = 4

    def __init__(self, port: int, world: int, rank: int, max_rows: int, path: str | None = None):
        import mmap

        self.world, self.rank, self.max_rows = world, rank, max_rows
        self.path = path or f"/dev/shm/ptts-serve-{port}-{world}.load"
        size = 8 * self.FIELDS * world
        fd = os.open(self.path, os.O_RDWR | os.O_CREAT, 0o600)
        try:
            if os.fstat(fd).st_size != size:
                os.ftruncate(fd, size)
            self._mm = mmap.mmap(fd, size)
        finally:
            os.close(fd)
        self.v = np.frombuffer(self._mm, np.int64).reshape(world, self.FIELDS)
        self.v[rank] = (0, 0, os.getpid(), self._start_time(os.getpid()))  # whatever an earlier run left
        self.private_port = 0

    def publish(self, load: int):
        self.v[self.rank, 0] = load

    def set_private_port(self, port: int):
        self.private_port = port
        self.v[self.rank, 1] = port

    @staticmethod
    def _start_time(pid: int) -> int:
        """The process's start time in clock ticks since boot (/proc/<pid>/stat field 22); -1 if
        there is no such process (0 where /proc is not available)."""
        try:
            with open(f"/proc/{int(pid)}/stat", "rb") as f:
                stat = f.read().decode(errors="replace")
        except FileNotFoundError:
            return -1
        except OSError:
            return 0
        # the command name (field 2) is parenthesised and may hold spaces: fields after its ')'
        return int(stat[stat.rindex(")") + 2:].split()[19])

    @classmethod
    def _alive(cls, pid: int, start: int = 0) -> bool:
        """True while the worker that published (pid, start) runs: a live process with that pid,
        owned by this user, started at that time (a reused pid has a later start time)."""
        if pid <= 0:
            return False
        try:
            os.kill(int(pid), 0)
        except ProcessLookupError:
            return False
        except PermissionError:  # exists, owned by another user: not one of this server's workers
            return False
        return start == 0 or cls._start_time(pid) == start

    def redirect_target(self, own_load: int) -> int | None:
        """The private port of the least-loaded live peer with a free slot, if this worker has none."""
        if own_load < self.max_rows:
            return None
        loads, ports, pids, starts = (self.v[:, i].copy() for i in range(self.FIELDS))
        best = None
        for r in range(self.world):
            if (r != self.rank and ports[r] > 0 and loads[r] < self.max_rows and (best is None or loads[r] < loads[best])
                    and self._alive(pids[r], starts[r])):
                best = r
        if best is None:
            return None
        self.v[best, 0] += 1  # claim the slot now: concurrent overflows spread instead of herding
        return int(ports[best])

    def close(self, unlink: bool = False):
        if self.v is not None:
            self.v[self.rank] = (0, 0, 0, 0)  # a closed worker is no target
        self.v = None
        self._mm.close()
        if unlink:
            try:
                os.unlink(self.path)
            except FileNotFoundError:
                pass


# ---------------------------------------------------------------------------------------------
def load_tokenizer(path: str) -> Callable[[str], list[int]]:
    """tokenizer.model (SentencePiece) or tokenizer.json; a .json file is read with the native
    Rust settings (text.rs:71-79: Metaspace prepend "always", no BOS), see text.py."""
    from .text import Tokenizer

    return Tokenizer.from_file(path, native=True)


_B64_ALPHABET = re.compile(r"[A-Za-z0-9+/=]+")
_DATA_URL = re.compile(r"data:audio/[^;,]*;base64,", re.ASCII)
_VOICE_NAME = re.compile(r"[A-Za-z0-9_.-]{1,64}")


def voice_spec_audio(spec: str) -> bytes | None:
    """The audio bytes of a base64 voice spec, by the reference's rule (voice.rs:172-222): a
    `data:audio/...;base64,` URL, or raw base64 (longer than 100 characters, base64 alphabet only);
    None for anything else. Nothing here touches the file system or the network."""
    spec = spec.strip()
    m = _DATA_URL.match(spec)
    if m:
        payload = spec[m.end():]
    elif len(spec) > 100 and _B64_ALPHABET.fullmatch(spec):
        payload = spec
    else:
        return None
    try:
        return base64.b64decode(payload, validate=True)
    except (binascii.Error, ValueError) as e:
        raise ValueError(f"voice: base64 audio does not decode ({e})") from e


def wav_wire_samples(data: bytes) -> tuple[np.ndarray, int]:
    """A mono RIFF/WAVE clip -> (samples in their wire format, sample rate): int16 where every
    sample is an int16 value / 32768 (8- and 16-bit PCM: the engine converts them on the GPU, the
    same numbers exactly), float32 otherwise. Raises ValueError (WavError) for anything else."""
    from .audio import read_wav_from_bytes

    x, sr = read_wav_from_bytes(data)
    if x.shape[0] != 1:
        raise ValueError(f"voice prompt must be mono, got {x.shape[0]} channels")
    if x.shape[1] < 1 or sr <= 0:
        raise ValueError("voice prompt holds no samples")
    y = x[0] * np.float32(32768.0)  # exact (a power of two)
    yi = y.astype(np.int16)
    if np.array_equal(yi, y):
        return yi, sr
    return np.ascontiguousarray(x[0], np.float32), sr


class _Calibration:
    """One clip's loudness calibration: `done` is set once `value` (LUFS, or None: unmeasurable) or
    `error` is in place."""

    def __init__(self):
        self.done, self.value, self.error = threading.Event(), None, None


class TTSService:
    """Request-level logic shared by the HTTP routes: text -> ids, voice lookup, params."""

    def __init__(self, scheduler, voices: dict[str, Voice | Sequence[Voice]], default_voice: str,
                 tokenizer: Callable[[str], Sequence[int]] | None = None, temp: float = 0.7,
                 eos_threshold: float = -4.0, noise_clamp: float | None = None, lsd_decode_steps: int = 1,
                 max_lsd_steps: int | None = None, max_voice_seconds: float = 30.0, voice_chunk_frames: int = 0,
                 voice_resampler: str = "poly", max_ctx: int | None = None, long_form: bool = False,
                 continuity: bool = False):
        """continuity: whether a text request that does not say runs its sentence chunks as a
        continuity chain (request(continuity=...); it implies the long-form cut).
        long_form: whether a text request that does not say is split into segments on parallel
        rows (request(long_form=...)).
        lsd_decode_steps: the Euler step count of a request that names none (the engine's own
        default). max_lsd_steps: the largest `lsd_steps` a request may ask for, the engine's cap
        (None: lsd_decode_steps, so any other value is refused). max_voice_seconds: longest clip a
        request (or POST /voices) may bring. voice_chunk_frames / voice_resampler: the clone
        settings of such clips (Engine.voice_job). max_ctx: the engines' context (a voice must be
        shorter), read from the scheduler's engine when not given."""
        self.max_voice_seconds = float(max_voice_seconds)
        self.voice_chunk_frames, self.voice_resampler = int(voice_chunk_frames), voice_resampler
        eng = getattr(scheduler, "engine", None) or getattr(getattr(scheduler, "schedulers", [None])[0], "engine", None)
        self.max_ctx = max_ctx if max_ctx is not None else getattr(eng, "max_ctx", None)
        self.wire = bool(getattr(eng, "wire", False))  # the engines convert to wire formats (--wire)
        self.tempo = self.wire and bool(getattr(eng, "tempo_enabled", False))  # and time-scale (--tempo)
        self.flac = self.wire and bool(getattr(eng, "flac_enabled", False))  # and encode FLAC (--flac)
        self.flac_join = self.flac and hasattr(eng, "fetch_flac_index")  # and say where a chunk's frames are
        self.pitch = self.tempo and bool(getattr(eng, "pitch_enabled", False))  # and shift the pitch (--pitch)
        self.level = self.wire and bool(getattr(eng, "level_enabled", False))  # and set the level (--volume)
        self.align = bool(getattr(eng, "align_enabled", False))  # and deliver alignment rows (--align)
        self.loud = self.wire and bool(getattr(eng, "loud_enabled", False))  # and meter loudness (--loudness)
        # calibrated loudness (LUFS; None: unmeasurable) of the registered voices by name and of
        # per-request clips by their key, the latter bounded like the clone cache
        self.voice_lufs: dict = {}
        self.clip_lufs: OrderedDict = OrderedDict()  # clip key -> _Calibration, under _cal_lock
        self._cal_lock = threading.Lock()
        sch0 = getattr(scheduler, "schedulers", [scheduler])[0]
        self._cal_capacity = max(int(getattr(getattr(sch0, "voices", None), "capacity", 64)), 1)
        self.scheduler = scheduler
        self.voices = voices
        self.default_voice = default_voice
        self.tokenizer = tokenizer
        self.temp, self.eos_threshold, self.noise_clamp = temp, eos_threshold, noise_clamp
        self.lsd_decode_steps = lsd_decode_steps
        self.max_lsd_steps = lsd_decode_steps if max_lsd_steps is None else max_lsd_steps
        self.long_form = bool(long_form)
        self.continuity = bool(continuity)
        self._seed = 0
        self._lock = threading.Lock()
        if self.loud:  # the voices the server starts with (--voice)
            for name in list(self.voices):
                self.voice_lufs[name] = self.calibrate(self.voices[name])

    def calibrate(self, target) -> float | None:
        """The loudness of a voice (a registered voice or a clip) in LUFS: the calibration sentence at
        the server's default parameters and a fixed seed, no gain, 24000 / pcm_s16le with the bytes
        discarded, metered; an ordinary request through the scheduler. None: unmeasurable (also a
        server with no tokenizer, which cannot say the sentence)."""
        if not self.loud or self.tokenizer is None:
            return None
        ids, mgl, fae = segment_request(CALIBRATION_TEXT, self.tokenizer)
        p = GenerationParams(temp=self.temp, eos_threshold=self.eos_threshold, noise_clamp=self.noise_clamp,
                             frames_after_eos=fae, max_frames=mgl, seed=CALIBRATION_SEED, sample_rate=SAMPLE_RATE,
                             encoding="pcm_s16le", loudness=True)
        r = self.scheduler.submit(np.asarray(ids, np.int32), target, p)
        r.wire_audio()
        return r.loudness()

    def clip_loudness(self, clip: VoiceClip) -> float | None:
        """The loudness of a per-request clip, calibrated on its first use and kept by the clip's key
        beside the clone caches: the same key, capacity and least-recently-used order (the caches
        themselves belong to the scheduler threads, one per engine). A second request that comes
        while the first still calibrates waits for that one run. Called from request threads."""
        with self._cal_lock:
            ent = self.clip_lufs.get(clip.key)
            mine = ent is None
            if mine:
                ent = self.clip_lufs[clip.key] = _Calibration()
                while len(self.clip_lufs) > self._cal_capacity:
                    self.clip_lufs.popitem(last=False)
            else:
                self.clip_lufs.move_to_end(clip.key)
        if not mine:
            ent.done.wait()
            if ent.error is not None:
                raise RuntimeError("the voice's calibration failed") from ent.error
            return ent.value
        try:
            ent.value = self.calibrate(clip)
        except BaseException as e:
            ent.error = e
            with self._cal_lock:
                if self.clip_lufs.get(clip.key) is ent:
                    del self.clip_lufs[clip.key]
            raise
        finally:
            ent.done.set()
        return ent.value

    def voice_info(self, name: str) -> dict:
        """GET /voices/NAME. KeyError: no such voice."""
        with self._lock:
            v = self.voices[name]
            lufs = self.voice_lufs.get(name)
        v0 = v[0] if isinstance(v, (list, tuple)) else v
        return {"name": name, "frames": int(getattr(v0, "n_frames", 0)), "loudness_lufs": lufs}

    def _count_tokens(self, text: str) -> int:
        tok = self.tokenizer
        return tok.count_tokens(text) if hasattr(tok, "count_tokens") else len(tok(text))

    def request(self, text: str | None = None, token_ids=None, voice: str | None = None,
                temperature: float | None = None, eos_threshold: float | None = None,
                noise_clamp: float | None = None, lsd_steps: int | None = None, words: int | None = None,
                max_frames: int | None = None, sample_rate: int | None = None,
                encoding: str | None = None, long_form: bool | None = None, speed: float | None = None,
                continuity: bool | None = None, pitch: float | None = None, volume_db: float | None = None,
                limit: bool | None = None, timestamps: bool | None = None, loudness_lufs: float | None = None,
                loudness: bool | None = None) -> Request:
        """loudness_lufs: a target in [-40, -5] LUFS: the rows get the constant gain target - the voice's
        calibrated loudness (within +-24 dB) through the level stage, limiter on; the gain is the
        returned object's gain_db. It excludes volume_db and needs --loudness and --volume.
        loudness: the rows are metered; loudness() of the returned object, once its audio is consumed,
        is the response's integrated loudness.
        timestamps: the rows also deliver their alignment rows, for words();
        a text request on a server with the align stage (--align), not with continuity (that row's
        text also holds the previous chunk's ids) and not with token_ids (they carry no words).
        volume_db: -24 .. 24 dB (rounded to hundredths), limit: run the row through the peak limiter
        even without a gain; the row's wire bytes are scaled and limited to the server's ceiling on the
        GPU (None / 0 and None / False: unchanged).
        continuity (None: the server's default, --continuity): the long-form
        cut, with the sentence chunks of a text piece generated one after another on one slot, each
        teacher-forced through the one before it and decoded on from its codec state, so prosody
        and the codec run across the joins. token_ids are never split, so they cannot ask for it.
        speed: 0.5 .. 2.0, the row's wire bytes time-scaled on the GPU (None or 1.0: unchanged).
        pitch: -12 .. 12 semitones, the row's wire bytes shifted in pitch on the GPU at the duration
        `speed` asks for (None or 0: unchanged).
        long_form (None: the server's default, --long-form): the text is split as the reference's
        routes split it (generate_stream_long: pause markers and natural pauses become silence,
        each text piece is cut into sentence chunks of at most 50 tokens) and the chunks run as
        rows of the batch, delivered in text order behind one Request-like object (RequestGroup).
        token_ids are never split."""
        if long_form and token_ids is not None:
            raise ValueError("long_form needs `text`: token_ids are never split")
        if continuity and token_ids is not None:
            raise ValueError("continuity needs `text`: token_ids are never split")
        chain = token_ids is None and (self.continuity if continuity is None else bool(continuity))
        if timestamps:
            if not self.align:
                raise ValueError("this server runs without the align stage (--align): timestamps are not available")
            if token_ids is not None:
                raise ValueError("timestamps need `text`: token_ids carry no words")
            if chain:
                raise ValueError("timestamps with continuity are not available: a continuing row's text also holds "
                                 "the previous chunk's ids"
                                 + (" (this server's default is --continuity: send `continuity: false`)"
                                    if continuity is None else ""))
            if encoding == "flac":
                raise ValueError("timestamps with flac are not available")
            if not hasattr(self.tokenizer, "pieces"):
                raise ValueError("timestamps need a tokenizer that names its pieces")
        if sample_rate is not None or encoding is not None:
            if sample_rate is not None and sample_rate not in WIRE_RATES:
                raise ValueError(f"sample_rate must be one of {list(WIRE_RATES)}")
            if encoding is not None and encoding not in ENCODINGS:
                raise ValueError(f"encoding must be one of {list(ENCODINGS)}")
            if not self.wire:
                raise ValueError("this server runs without wire output (--no-wire): sample_rate / encoding "
                                 "are not available")
        if encoding == "flac":
            if not self.flac:
                raise ValueError("this server runs without the FLAC stage (--no-flac or --no-wire): encoding flac is "
                                 "not available")
            if not self.flac_join and (chain or (token_ids is None and (self.long_form if long_form is None else long_form))):
                raise ValueError("flac with long_form or continuity is not available: the segments of one response "
                                 "are separate rows, each numbering its samples from 0, and this engine has no frame "
                                 "index to renumber them by")
        if limit is not None and not isinstance(limit, (bool, np.bool_)):
            raise ValueError(f"limit must be a bool, got {limit!r}")
        if loudness is not None and not isinstance(loudness, (bool, np.bool_)):
            raise ValueError(f"loudness must be a bool, got {loudness!r}")
        if loudness and not self.loud:
            raise ValueError("this server runs without the loudness stage (--loudness): loudness is not available")
        gain_db = None
        if loudness_lufs is not None:  # (the gain itself: below, once everything else about the request is valid)
            if not (math.isfinite(float(loudness_lufs)) and -40.0 <= float(loudness_lufs) <= -5.0):
                raise ValueError(f"loudness_lufs must be in [-40, -5] LUFS, got {loudness_lufs!r}")
            if volume_db is not None:
                raise ValueError("loudness_lufs and volume_db exclude each other")
            if not (self.loud and self.level):
                raise ValueError("this server runs without the loudness stage or the level stage (--loudness, "
                                 "--volume): loudness_lufs is not available")
        # (ValueError: a value out of range); a field that changes nothing is the request without it
        out = OutputOptions.of(sample_rate, encoding, speed, pitch, volume_db, limit)
        if out.speed is not None and not self.tempo:
            raise ValueError("this server runs without the tempo stage (--no-tempo or --no-wire): speed is not "
                             "available")
        if out.pitch is not None and not self.pitch:
            raise ValueError("this server runs without the pitch stage (--no-pitch, --no-tempo or --no-wire): "
                             "pitch is not available")
        if out.volume_db is not None and not self.level:
            raise ValueError("this server runs without the level stage (--no-volume or --no-wire): volume_db / "
                             "limit are not available")
        if lsd_steps is not None and not 1 <= lsd_steps <= self.max_lsd_steps:
            raise ValueError(f"lsd_steps must be in [1, {self.max_lsd_steps}], the engine's cap (--max-lsd-steps); "
                             f"the default is {self.lsd_decode_steps}")
        segments = None
        if token_ids is not None:  # extension: ids carry no word count, the client states it
            ids = np.asarray(token_ids, np.int32).reshape(-1)
            if words is None and max_frames is None:
                raise ValueError("token_ids need `words` (word count of their text) or `max_frames`")
            mgl = max_frames or (words + 2) * 13
            fae = 3 if words is None else (5 if words <= 4 else 3)
        elif text is not None:
            if self.tokenizer is None:
                raise ValueError("no tokenizer configured: send token_ids")
            if chain or (self.long_form if long_form is None else long_form):
                segments = []  # ("text", ids, max_frames, frames_after_eos) | ("pause", ms), in text order
                for kind, val in long_form_segments(text, self._count_tokens, pauses=True):
                    if kind == "text":
                        sid, mgl, fae = segment_request(val, self.tokenizer)
                        segments.append(("text", np.asarray(sid, np.int32), max_frames or mgl, fae))
                    else:
                        segments.append((kind, val))
            else:
                prepared = prepare_text_prompt(text)
                ids = np.asarray(self.tokenizer(prepared), np.int32)
                mgl, fae = max_frames or max_gen_len(prepared), estimate_frames_after_eos(text)
        else:
            raise ValueError("text or token_ids required")
        if timestamps:  # refused here, not by the engine: its refusal fails a whole batched admission
            longest = max((sg[1].size for sg in segments if sg[0] == "text"), default=0) if segments is not None \
                else ids.size
            if longest > ALIGN_TOKENS:
                raise ValueError(f"timestamps: a row of {longest} tokens exceeds the align stage's {ALIGN_TOKENS}"
                                 + ("" if segments is not None else " (send `long_form: true`: every sentence chunk "
                                                                    "is a row of at most 50 tokens)"))
        name = voice or self.default_voice
        # not a registered name: base64 audio (decoded outside the lock), or refused
        clip = None if name in self.voices else self.voice_clip(name)
        if loudness_lufs is not None:  # the last check: a per-request clip's calibration is a generation
            cal = self.clip_loudness(clip) if clip is not None else self.voice_lufs.get(name)
            if cal is None:
                raise ValueError("the voice's loudness is unmeasurable: no loudness target for it")
            gain_db = loudness_gain_cdb(float(loudness_lufs), cal) / 100.0
            out = OutputOptions.of(sample_rate, encoding, speed, pitch, gain_db, True)
        # the name is resolved and the request queued under the lock register_voice swaps the name
        # under: a replaced voice is retired only after every request that got it is queued, and
        # the scheduler closes it only once none of them is still waiting (BatchScheduler.retire)
        with self._lock:
            target = clip if clip is not None else self.voices[name]
            if segments is not None:  # one seed per text segment, in text order
                segs = [("text", sg[1], self._params_locked(temperature, eos_threshold, noise_clamp, sg[3], sg[2],
                                                            lsd_steps, out, bool(timestamps), bool(loudness)))
                        if sg[0] == "text" else sg for sg in segments]
                # (pauses: silence of their stated duration in the rows' format, whatever the speed)
                if chain:
                    r = self.scheduler.submit_group(segs, target, out.wire, continuity=True)
                else:
                    r = self.scheduler.submit_group(segs, target, out.wire)
            else:
                r = self._submit_locked(ids, target, temperature, eos_threshold, noise_clamp, fae, mgl, lsd_steps,
                                        out, bool(timestamps), bool(loudness))
        if gain_db is not None:
            r.gain_db = gain_db
        return r

    def words(self, r) -> list[dict]:
        """[{"word", "start", "end"}] of a finished timestamps request (its audio consumed), in seconds
        of the audio delivered: align.timestamps per text segment, each offset by the samples handed
        over before it (a long-form request's pauses included)."""
        from . import align as _align

        rate = r.wire[0] if r.wire else SAMPLE_RATE
        out, at = [], 0
        for it in (r.items if isinstance(r, RequestGroup) else [r]):
            if not isinstance(it, Request):
                at += item_samples(it, r.wire)
                continue
            p, n = it.params, len(it.align_rows or [])
            A = np.zeros((n, it.ids.size), np.float64)
            for t, row in enumerate(it.align_rows or []):
                A[t, :min(row.size, it.ids.size)] = row[:it.ids.size]
            eos = max(n - p.frames_after_eos, 0) if n < p.max_frames else None
            for w in _align.timestamps(self.tokenizer, it.ids, A, p.speed or 1.0, eos, it.units / rate):
                out.append({"word": w["word"], "start": round(w["start"] + at / rate, 6),
                            "end": round(w["end"] + at / rate, 6)})
            at += it.units
        return out

    def _submit_locked(self, ids, target, temperature, eos_threshold, noise_clamp, fae, mgl, lsd_steps,
                       out=OutputOptions(), align=False, loud=False) -> Request:
        p = self._params_locked(temperature, eos_threshold, noise_clamp, fae, mgl, lsd_steps, out, align, loud)
        return self.scheduler.submit(ids, target, p)  # MultiGpuScheduler: one voice per GPU, or the clip

    def _params_locked(self, temperature, eos_threshold, noise_clamp, fae, mgl, lsd_steps, out=OutputOptions(),
                       align=False, loud=False) -> GenerationParams:
        self._seed += 1
        seed = self._seed
        p = GenerationParams(temp=self.temp if temperature is None else temperature,
                             eos_threshold=self.eos_threshold if eos_threshold is None else eos_threshold,
                             noise_clamp=self.noise_clamp if noise_clamp is None else noise_clamp,
                             frames_after_eos=fae, max_frames=mgl, seed=seed,
                             lsd_steps=None if lsd_steps is None else int(lsd_steps), align=bool(align))
        if loud:  # (set only then: a request without it submits the params of before)
            p.loudness = True
        return out.apply(p)

    # -- per-request and run-time voices
    def voice_clip(self, spec: str) -> VoiceClip:
        """The `voice` field of a request that names no registered voice -> the clip to clone.
        ValueError (HTTP 400) for anything but base64 WAV audio: unknown names, and the file paths
        and hf:// specs the reference would resolve (deliberately not accepted from the network)."""
        data = voice_spec_audio(spec)
        if data is None:
            shown = spec if len(spec) <= 64 else spec[:61] + "..."
            raise ValueError(f"unknown voice {shown!r} (a registered name or base64 WAV audio; file paths and "
                             "hf:// specs are not accepted)")
        return self.wav_clip(data)

    def wav_clip(self, data: bytes) -> VoiceClip:
        samples, sr = wav_wire_samples(data)
        if samples.size > self.max_voice_seconds * sr:
            raise ValueError(f"voice prompt is {samples.size / sr:.1f} s long, the limit is "
                             f"{self.max_voice_seconds:g} s (--max-voice-seconds)")
        frames = clip_frames(samples.size, sr, self.voice_resampler)
        if frames < 1 or (self.max_ctx is not None and frames >= self.max_ctx):
            raise ValueError(f"voice prompt of {frames} frames does not fit the engine's context")
        h = hashlib.blake2b(data, digest_size=16)
        h.update(f"|chunk={self.voice_chunk_frames}|resampler={self.voice_resampler}".encode())
        return VoiceClip(h.digest(), frames, samples, sr, self.voice_chunk_frames, self.voice_resampler)

    def prompt_clip(self, data: bytes) -> VoiceClip:
        """A safetensors file holding `audio_prompt` [.. x F x 1024] (the reference's voice embeddings)."""
        from safetensors.numpy import load as st_load

        try:
            t = st_load(data)
        except Exception as e:
            raise ValueError(f"body is neither RIFF/WAVE nor safetensors ({e})") from e
        if "audio_prompt" not in t or t["audio_prompt"].size == 0 or t["audio_prompt"].shape[-1] != 1024:
            raise ValueError("safetensors body needs an `audio_prompt` tensor [F x 1024]")
        prompt = np.ascontiguousarray(t["audio_prompt"], np.float32).reshape(-1, 1024)
        if self.max_ctx is not None and prompt.shape[0] >= self.max_ctx:
            raise ValueError(f"audio_prompt of {prompt.shape[0]} frames does not fit the engine's context")
        return VoiceClip(hashlib.blake2b(data, digest_size=16).digest(), prompt.shape[0], prompt=prompt)

    def register_voice(self, name: str, data: bytes) -> int:
        """POST /voices/{name}: clone `data` (WAV clip or safetensors audio_prompt) on every engine,
        each on its scheduler thread, and register (or replace) the named voice. The registry owns
        these voices: they are outside the LRU cache. Returns the voice's frames."""
        if not _VOICE_NAME.fullmatch(name):
            raise ValueError("voice name must be 1-64 characters of [A-Za-z0-9_.-]")
        clip = self.wav_clip(data) if data[:4] == b"RIFF" else self.prompt_clip(data)
        scheds = getattr(self.scheduler, "schedulers", None)
        if scheds is None:
            new = self.scheduler.call(lambda: clip.start(self.scheduler.engine))
        else:
            new = [s.call(lambda s=s: clip.start(s.engine)) for s in scheds]
        lufs = self.calibrate(new) if self.loud else None  # (before the swap: the name never lacks its value)
        with self._lock:
            old, self.voices[name] = self.voices.get(name), new
            if self.loud:
                self.voice_lufs[name] = lufs
        if old is not None:  # closed once no queued request holds it; rows reading it keep it alive
            if scheds is None:
                self.scheduler.retire(old)
            else:
                for s, v in zip(scheds, old):
                    s.retire(v)
        return clip.n_frames

    def voice_names(self) -> list[str]:
        with self._lock:
            return sorted(self.voices)


from pydantic import BaseModel  # noqa: E402  (request bodies; module level so FastAPI resolves them)
from starlette.requests import Request as StarletteRequest  # noqa: E402


class GenerateRequest(BaseModel):
    """handlers.rs:84-92 (+ token_ids when no tokenizer is configured)."""

    text: str | None = None
    token_ids: list[int] | None = None
    words: int | None = None  # with token_ids: word count of their text (max_gen_len rule)
    max_frames: int | None = None
    voice: str | None = None
    temperature: float | None = None
    lsd_steps: int | None = None
    eos_threshold: float | None = None
    noise_clamp: float | None = None
    # wire format (converted on the GPU): 8000 / 16000 / 24000 / 44100 / 48000 and pcm_s16le / ulaw /
    # alaw; one of them alone defaults the other to 24000 / pcm_s16le; neither: today's output
    sample_rate: int | None = None
    encoding: str | None = None
    # speech speed, 0.5 .. 2.0 (time-scaled on the GPU, pitch kept); unset or 1.0: unchanged
    speed: float | None = None
    # pitch shift in semitones, -12 .. 12 (resampled on the GPU at the duration `speed` asks for; formants
    # move with the fundamental); unset or 0: unchanged
    pitch: float | None = None
    # volume in dB, -24 .. 24, and `limit`: the look-ahead peak limiter even with no gain (both on the GPU,
    # behind speed and pitch); unset, or 0 with limit unset: unchanged
    volume_db: float | None = None
    limit: bool | None = None
    # loudness target in LUFS, -40 .. -5 (a constant gain from the voice's calibrated loudness, limiter on;
    # excludes volume_db), and `loudness`: meter the response (X-Loudness-LUFS); DESIGN.md section 27
    loudness_lufs: float | None = None
    loudness: bool | None = None
    # split the text into segments on parallel rows, pauses as silence (None: the server's --long-form)
    long_form: bool | None = None
    # the long-form cut with each sentence chunk continuing the one before it (None: --continuity)
    continuity: bool | None = None
    # word timestamps (a server with --align; not on /stream): the answer is JSON, the audio in base64
    timestamps: bool | None = None


class OpenAIRequest(BaseModel):
    """handlers.rs:378-385."""

    model: str = "pocket-tts"
    input: str | None = None
    voice: str | None = None
    response_format: str | None = None  # wav (default), pcm, flac, ulaw, alaw (raw G.711, 8 kHz unless sample_rate)
    token_ids: list[int] | None = None
    words: int | None = None
    sample_rate: int | None = None
    encoding: str | None = None
    speed: float | None = None  # 0.5 .. 2.0, as in the API this route imitates (0.25 .. 4.0 there)
    pitch: float | None = None  # -12 .. 12 semitones (no counterpart in that API)
    volume_db: float | None = None  # -24 .. 24 dB (no counterpart in that API)
    limit: bool | None = None
    # loudness target in LUFS, -40 .. -5 (a constant gain from the voice's calibrated loudness, limiter on;
    # excludes volume_db), and `loudness`: meter the response (X-Loudness-LUFS); DESIGN.md section 27
    loudness_lufs: float | None = None
    loudness: bool | None = None
    long_form: bool | None = None
    continuity: bool | None = None
    timestamps: bool | None = None  # as in GenerateRequest


# /stream: at most one chunk per stream per 20 ms after the first (32 streams x 50 wakes/s keep the
# event loop, which shares the GIL with the scheduler thread, well below one core)
CHUNK_INTERVAL_S = 0.02


async def pcm_chunks(r: Request):
    """/stream body without a worker thread per stream. The driver's put() wakes this coroutine
    on the event loop (call_soon_threadsafe, at most one pending wake per stream); each wake
    sends every frame available at that moment as ONE chunk of 16-bit PCM, then the stream
    waits CHUNK_INTERVAL_S before the next. The first frame goes out as soon as it exists; later
    frames coalesce, so 32 streams of a GPU producing ~4000x real time cost at most 50 chunks/s
    each instead of one event-loop round trip per 80-ms frame (which throttled the whole server).
    """
    import asyncio

    loop = asyncio.get_running_loop()
    ev = asyncio.Event()
    armed = [False]

    def wake():
        if armed[0]:
            armed[0] = False
            loop.call_soon_threadsafe(ev.set)

    r.waker = wake
    done = False
    try:
        while True:
            items = []
            while True:
                try:
                    items.append(r.out.get_nowait())
                except queue.Empty:
                    break
            batch = []
            for item in items:
                if item is None:
                    done = True
                    break
                if isinstance(item, BaseException):
                    done = True  # the request has ended on the scheduler's side
                    raise item
                batch.append(item)
            if batch:
                if "chunk0" not in r.times:
                    r.times["chunk0"] = time.time()
                if isinstance(batch[0], bytes):  # a wire request: the engine's bytes, untouched
                    yield batch[0] if len(batch) == 1 else b"".join(batch)
                else:
                    yield pcm_i16_le_bytes(batch[0] if len(batch) == 1 else np.concatenate(batch))
            if done:
                return
            if batch:
                await asyncio.sleep(CHUNK_INTERVAL_S)
            ev.clear()
            armed[0] = True
            if r.out.empty():
                await ev.wait()
    finally:
        # closed before the end marker (GeneratorExit / CancelledError): the client went away, so
        # its rows stop now instead of running to EOS or max_frames
        if not done and hasattr(r, "cancel"):
            r.cancel()


async def flac_chunks(r: Request):
    """/stream body of a FLAC request: the stream header (sample count unknown), then pcm_chunks (a
    group's items are already renumbered: RequestGroup._pump)."""
    yield flac_stream_header(r.wire[0])
    async for chunk in pcm_chunks(r):
        yield chunk


def flac_file(r) -> bytes:
    """A FLAC request's whole output as a file: the header with the true sample count (one item per
    frame of the row, whatever its size; a group's joiner has counted), then the chunks untouched."""
    chunks = list(r.stream())
    joiner = getattr(r, "joiner", None)
    if joiner is not None:
        return flac_stream_header(r.wire[0], joiner.total) + b"".join(chunks)
    total = wire_samples(len(chunks) * FRAME, r.wire[0], getattr(r, "speed", 0), getattr(r, "pitch", 0))
    return flac_stream_header(r.wire[0], total) + b"".join(chunks)


def create_app(service: TTSService):
    from fastapi import FastAPI, HTTPException
    from fastapi.responses import JSONResponse, Response, StreamingResponse

    app = FastAPI(title="pocket-tts (MI355X engine)")

    def submit(**kw) -> Request:
        try:
            return service.request(**kw)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e)) from e

    def timed(r, data: bytes, media: str, metered=False):
        """The answer of a timestamps request: what the route would have sent, in base64, and the words."""
        body = {"audio": base64.b64encode(data).decode(), "content_type": media,
                "sample_rate": r.wire[0] if r.wire else SAMPLE_RATE, "words": service.words(r)}
        if metered:
            body["loudness_lufs"] = r.loudness()
        return JSONResponse(body, headers=loud_headers(r, metered))

    worker = getattr(service, "worker", None) or {"rank": 0, "world": 1, "pid": os.getpid()}
    hdr = {"X-PTTS-Rank": str(worker["rank"])}
    board: LoadBoard | None = getattr(service, "board", None)
    shared_port = getattr(service, "shared_port", None)

    def overflow(request):
        """A 307 to the least-loaded peer's private port when this worker has no free slot and the
        request came in on the shared port (LoadBoard); None to serve it here."""
        if board is None or request.scope.get("server", (None, None))[1] != shared_port:
            return None
        from fastapi.responses import RedirectResponse

        port = board.redirect_target(service.scheduler.load())
        if port is None:
            return None
        return RedirectResponse(str(request.url.replace(port=port)), status_code=307, headers=hdr)

    @app.get("/health")
    def health():
        sch = getattr(service, "scheduler", None)
        stats = {"steps": sch.steps, "frames": sch.row_frames} if isinstance(sch, BatchScheduler) else {}
        return JSONResponse({"status": "healthy", "version": VERSION, "worker": worker, **stats}, headers=hdr)

    @app.get("/voices")
    def list_voices():
        return JSONResponse({"voices": service.voice_names(), "default": service.default_voice}, headers=hdr)

    @app.get("/voices/{name}")
    def voice_info(name: str):
        try:
            return JSONResponse(service.voice_info(name), headers=hdr)
        except KeyError:
            raise HTTPException(status_code=404, detail=f"no voice {name!r}") from None

    def loud_headers(r, metered) -> dict:
        """X-Gain-dB of a loudness_lufs request; X-Loudness-LUFS of a metered one (its audio consumed)."""
        h = dict(hdr)
        if getattr(r, "gain_db", None) is not None:
            h["X-Gain-dB"] = f"{r.gain_db:.2f}"
        if metered:
            v = r.loudness()
            h["X-Loudness-LUFS"] = "none" if v is None else f"{v:.2f}"
        return h

    @app.post("/voices/{name}")
    async def register_voice(name: str, request: StarletteRequest):
        from starlette.concurrency import run_in_threadpool

        body = await request.body()
        try:
            frames = await run_in_threadpool(service.register_voice, name, body)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e)) from e
        return JSONResponse({"voice": name, "frames": frames}, headers=hdr)

    @app.post("/generate")
    def generate(req: GenerateRequest, request: StarletteRequest):
        redirect = overflow(request)
        if redirect is not None:
            return redirect
        r = submit(**req.model_dump())
        if r.wire is not None and r.wire[1] == "flac":
            data = flac_file(r)
            return Response(data, media_type="audio/flac", headers=loud_headers(r, req.loudness))
        data = wav_bytes(r.wire_audio(), *r.wire) if r.wire is not None else wav_bytes(r.audio())
        if req.timestamps:
            return timed(r, data, "audio/wav", req.loudness)
        return Response(data, media_type="audio/wav", headers=loud_headers(r, req.loudness))

    @app.post("/stream")
    async def stream(req: GenerateRequest, request: StarletteRequest):
        t_route = time.time()
        redirect = overflow(request)
        if redirect is not None:
            return redirect
        if req.timestamps:
            raise HTTPException(status_code=400, detail="timestamps are not available on /stream: ask /generate")
        if req.loudness:
            raise HTTPException(status_code=400, detail="loudness is not available on /stream (a stream has no place "
                                                        "for the value): ask /generate")
        if req.loudness_lufs is not None:  # may calibrate an inline clip, a whole generation: not on the event loop
            from starlette.concurrency import run_in_threadpool

            r = await run_in_threadpool(lambda: submit(**req.model_dump()))
        else:
            r = submit(**req.model_dump())
        r.times["route"] = t_route
        sh = {**loud_headers(r, False), "X-PTTS-Route-Time": f"{t_route:.6f}"}  # (the gain is known at admission)
        if r.wire is not None and r.wire[1] == "flac":
            return StreamingResponse(flac_chunks(r), media_type="audio/flac", headers=sh)
        media = {"ulaw": "audio/PCMU", "alaw": "audio/PCMA"}.get(r.wire[1] if r.wire else "", "audio/pcm")
        return StreamingResponse(pcm_chunks(r), media_type=media, headers=sh)

    @app.post("/v1/audio/speech")
    def openai_speech(req: OpenAIRequest, request: StarletteRequest):
        redirect = overflow(request)
        if redirect is not None:
            return redirect
        fmt = req.response_format or "wav"
        rate, enc = req.sample_rate, req.encoding
        if fmt in ("ulaw", "alaw"):  # raw G.711: telephony's 8 kHz unless the request names a rate
            if enc not in (None, fmt):
                raise HTTPException(status_code=400, detail=f"response_format {fmt} contradicts encoding {enc}")
            rate, enc = rate or 8000, fmt
        elif fmt == "flac":
            if enc not in (None, fmt):
                raise HTTPException(status_code=400, detail=f"response_format {fmt} contradicts encoding {enc}")
            enc = fmt
        elif fmt == "pcm" and enc not in (None, "pcm_s16le"):
            raise HTTPException(status_code=400, detail=f"response_format pcm contradicts encoding {enc}")
        r = submit(text=req.input, token_ids=req.token_ids, voice=req.voice, words=req.words, sample_rate=rate,
                   encoding=enc, long_form=req.long_form, speed=req.speed, continuity=req.continuity, pitch=req.pitch,
                   volume_db=req.volume_db, limit=req.limit, timestamps=req.timestamps,
                   loudness_lufs=req.loudness_lufs, loudness=req.loudness)
        if r.wire is not None and r.wire[1] == "flac":
            data = flac_file(r)
            return Response(data, media_type="audio/flac", headers=loud_headers(r, req.loudness))
        if r.wire is not None:
            data = r.wire_audio()
            if fmt not in ("pcm", "ulaw", "alaw"):  # wav, and (as before) anything else
                data, media = wav_bytes(data, *r.wire), "audio/wav"
            else:
                media = {"ulaw": "audio/PCMU", "alaw": "audio/PCMA"}.get(r.wire[1], "audio/pcm")
        else:
            audio = r.audio()
            data, media = (pcm_i16_le_bytes(audio), "audio/pcm") if fmt == "pcm" else (wav_bytes(audio), "audio/wav")
        if req.timestamps:
            return timed(r, data, media, req.loudness)
        return Response(data, media_type=media, headers=loud_headers(r, req.loudness))

    return app


def stand_in_sample(u: int, k: int) -> float:
    """The stand-in engine's sample value for utterance u (its first token id) at frame k: the
    16-bit wire value (audio.rs:110-185: x 32767, truncated) is exactly (u % 128) * 256 + k % 256."""
    return ((u % 128) * 256 + k % 256 + 0.5) / 32767.0


def stand_in_align_row(k: int, frames: int, n: int) -> np.ndarray:
    """The stand-in engine's alignment row of frame k of a row of `frames` frames over n tokens: a
    band, 0.9 on token min(n - 1, k * n // frames) and 0.1 spread over all n."""
    a = np.full(n, 0.1 / max(n, 1), np.float32)
    if n:
        a[min(n - 1, k * n // max(frames, 1))] += np.float32(0.9)
    return a


@dataclass
class _StandInWire:
    """A wire row of the stand-in engine."""

    enc: str                 # encoding name
    level: tuple             # (gain_cdb, limit); (0, 0): not in the level stage
    u: int                   # the utterance (its first token id)
    total: int               # max_frames
    k: int = 0               # frames so far
    chunks: list | None = None        # a level row's chunks by the streaming host rule (computed once)
    last: np.ndarray | None = None    # the f32 chunk the latest bytes were made of: what a metered row's meter reads


class StandInEngine:
    """--stand-in-engine only (CPU; launcher and routing self-test of the multi-process server): the
    engine surface the scheduler drives, computing nothing. Row frames of utterance u (its first
    token id) at step k hold stand_in_sample(u, k), delivered one call late as by a pipelined
    engine; step_s paces each step (sleep) like a GPU step. level=True (with wire=True): the wire
    surface at 24 kHz and the level stage, by the host rule audio.level_limit over the row's frames;
    every admitted row's GenerationParams are kept in `params_log`."""

    def __init__(self, max_slots=32, max_ctx=1024, step_s=0.0, wire=False, level=False, level_ceiling_db=-1.0,
                 align=False, loud=False, **_):
        self.max_slots, self.max_ctx, self.pipeline = max_slots, max_ctx, True
        # loud=True (with wire=True): rows admitted with GenerationParams.loudness deliver, through
        # fetch_loud, the host rule's sub-block energies (audio.LoudnessMeter) over what their wire
        # stage reads, one call late like the frames
        self.loud_enabled = bool(wire and loud)
        self.meter = {}  # slot -> the row's LoudnessMeter
        self.loud_pending = self.loud_out = self.loud_prev = None
        # align=True: rows admitted with GenerationParams.align deliver a planted alignment row per
        # frame (stand_in_align_row) through fetch_align, one call late like the frames
        self.align_enabled = bool(align)
        self.arow = {}  # slot -> tokens of a row in the align stage
        self.align_pending = self.align_out = self.align_prev = None
        self.step_s = step_s
        self.rows, self.pending = {}, None
        self.admit_log = []  # every admitted row: (slot, ids, prefix latents or None, keep_codec)
        self.params_log = []  # and its GenerationParams
        self.level_enabled = bool(wire and level)
        self.level_ceiling_cdb = level_cdb(level_ceiling_db, -40.0, 0.0, "level_ceiling_db") if self.level_enabled else 0
        if self.level_enabled or self.loud_enabled:  # (without them the stand-in has no wire surface, as before)
            self.wire = True
        self.fmt = {}  # slot -> _StandInWire of a wire row
        self.wire_pending = self.wire_out = self.wire_prev = None

    @staticmethod
    def weight_blob_bytes():
        return 4096

    def finalize(self):
        pass

    def voice_from_prompt(self, prompt):
        from types import SimpleNamespace

        return SimpleNamespace(n_frames=int(np.asarray(prompt).shape[0]))

    class _Voice:
        def __init__(self, n_frames):
            self.n_frames, self.closed = int(n_frames), False

        def ready(self, wait=False):
            return True

        def close(self):
            self.closed = True

    def voice_job(self, samples, sample_rate, chunk_frames=0, resampler="poly"):
        """Counts the clones (voice_jobs) and checks what the engine checks on the host."""
        x = np.asarray(samples)
        if x.ndim != 1 or x.size < 1 or x.dtype not in (np.int16, np.float32) or sample_rate <= 0:
            raise ValueError("voice_job: a mono int16 / float32 clip at a positive rate")
        frames = clip_frames(x.size, sample_rate, "poly")
        if frames >= self.max_ctx:
            raise ValueError("voice prompt longer than max_ctx")
        self.voice_jobs = getattr(self, "voice_jobs", 0) + 1
        return self._Voice(frames)

    def voice_job_prompt(self, prompt):
        self.voice_jobs = getattr(self, "voice_jobs", 0) + 1
        return self._Voice(np.asarray(prompt).reshape(-1, 1024).shape[0])

    def reserve_voice_jobs(self, max_frames):
        self.voice_frames_reserved = int(max_frames)

    def open_many(self, slots, voices, ids_list, params_list):
        """Records every admitted row in `admit_log`; the latents of admission a's frame k hold a * 1000 + k."""
        for ids, p in zip(ids_list, params_list):  # as the engine: more than PTTS_ALIGN_TOKENS ids with align
            if getattr(p, "align", False) and len(ids) > ALIGN_TOKENS:
                raise RuntimeError("align: more than PTTS_ALIGN_TOKENS token ids")
        for p in params_list:  # nothing is admitted if one row is refused
            out = row_output(p)
            lv = out.codes()[4:]
            if lv != (0, 0) and not self.level_enabled:
                raise RuntimeError("a gain or limit needs a level-enabled engine")
            if getattr(p, "align", False) and not self.align_enabled:
                raise RuntimeError("align needs an align-enabled engine")
            if getattr(p, "loudness", False) and not self.loud_enabled:
                raise RuntimeError("loud needs a loudness-enabled engine")
            if out.wire and not ((self.level_enabled or self.loud_enabled) and out.wire[0] == SAMPLE_RATE and out.wire[1] != "flac"):
                raise RuntimeError("the stand-in engine converts to 24 kHz pcm_s16le / ulaw / alaw only, with level=True")
        for s, ids, p in zip(slots, ids_list, params_list):
            pre = getattr(p, "prefix_latents", None)
            self.params_log.append(p)
            self.fmt.pop(s, None)
            self.arow.pop(s, None)
            self.meter.pop(s, None)
            if getattr(p, "align", False):
                self.arow[s] = len(ids)
            out = row_output(p)
            if getattr(p, "loudness", False):
                self.meter[s] = LoudnessMeter()
            if out.wire or s in self.meter:  # (a metered row with no format: 24000 / pcm_s16le, as the engine's)
                self.fmt[s] = _StandInWire((out.wire or (SAMPLE_RATE, "pcm_s16le"))[1], out.codes()[4:],
                                           int(ids[0]) if len(ids) else 0, p.max_frames)
            self.rows[s] = [int(ids[0]) if len(ids) else 0, 0, p.max_frames, len(self.admit_log)]
            self.admit_log.append((int(s), [int(i) for i in ids], None if pre is None else np.array(pre, np.float32),
                                  bool(getattr(p, "keep_codec", False))))
            if self.pending is not None and s < self.pending[1].size:  # drop the slot's undrained frame
                self.pending[1][s] = False
                if self.wire_pending is not None and s < len(self.wire_pending):
                    self.wire_pending[s] = b""

    def cancel_slots(self, slots):
        """Engine.cancel_slots: the rows stop and no frame of theirs is reported any more."""
        self.cancelled = getattr(self, "cancelled", []) + [sorted(int(s) for s in slots)]
        for s in slots:
            self.rows.pop(s, None)
            self.fmt.pop(s, None)
            self.arow.pop(s, None)
            self.meter.pop(s, None)
            for held in (self.loud_pending, self.loud_out, self.loud_prev):
                if held is not None and s < len(held):
                    held[s] = np.zeros(0, np.float64)
            for held in (self.align_pending, self.align_out, self.align_prev):
                if held is not None and s < len(held):
                    held[s] = np.zeros(0, np.float32)
            for held in (self.wire_pending, self.wire_out, self.wire_prev):
                if held is not None and s < len(held):
                    held[s] = b""
            for held in (self.pending, getattr(self, "out", None), getattr(self, "prev_out", None)):
                if held is not None and s < held[1].size:
                    held[1][s] = False

    def step_async(self, n):
        if self.step_s:
            time.sleep(self.step_s)
        pcm, valid, last = np.zeros((n, FRAME), np.float32), np.zeros(n, bool), np.zeros(n, bool)
        lat = np.zeros((n, LDIM), np.float32)
        wire = [b""] * n
        arows = [np.zeros(0, np.float32)] * n
        lrows = [np.zeros(0, np.float64)] * n
        for s, st in list(self.rows.items()):
            if s < n:
                pcm[s], valid[s] = stand_in_sample(st[0], st[1]), True
                if s in self.arow:
                    arows[s] = stand_in_align_row(st[1], st[2], self.arow[s])
                if s in self.fmt:
                    wire[s] = self._wire_chunk(self.fmt[s])
                    if s in self.meter:  # what the wire stage read for the frame
                        lrows[s] = self.meter[s].feed(self.fmt[s].last)
                lat[s] = st[3] * 1000 + st[1]
                st[1] += 1
                last[s] = st[1] == st[2]
                if last[s]:
                    del self.rows[s]
        prev, self.pending = self.pending, (pcm, valid, last, lat)
        lprev, self.loud_pending = self.loud_pending, lrows
        self.loud_prev, self.loud_out = self.loud_out, [np.zeros(0, np.float64)] * n
        if lprev is not None:
            self.loud_out[:min(n, len(lprev))] = lprev[:min(n, len(lprev))]
        aprev, self.align_pending = self.align_pending, arows
        self.align_prev, self.align_out = self.align_out, [np.zeros(0, np.float32)] * n
        if aprev is not None:
            self.align_out[:min(n, len(aprev))] = aprev[:min(n, len(aprev))]
        wprev, self.wire_pending = self.wire_pending, wire
        self.wire_prev, self.wire_out = self.wire_out, [b""] * n
        if wprev is not None:
            self.wire_out[:min(n, len(wprev))] = wprev[:min(n, len(wprev))]
        self.prev_out = getattr(self, "out", None)
        self.out = (np.zeros((n, FRAME), np.float32), np.zeros(n, bool), np.zeros(n, bool),
                    np.zeros((n, LDIM), np.float32))
        if prev is not None:  # the previous call's frame, over this call's rows
            m = min(n, prev[1].size)
            for a, b in zip(self.out, prev):
                a[:m] = b[:m]

    def sync(self):
        pass

    def fetch(self, n, calls_back=0):
        from types import SimpleNamespace

        out = self.out if calls_back == 0 else self.prev_out
        return SimpleNamespace(pcm=out[0], valid=out[1], last=out[2], latents=out[3])

    def _wire_chunk(self, f) -> bytes:
        """The next wire chunk of a wire row: its frame's bytes, or for a level row the frame's chunk
        of the streaming host rule over the row's whole signal (computed once)."""
        k = f.k
        f.k = k + 1
        if f.level == (0, 0):
            x = np.full(FRAME, stand_in_sample(f.u, k), np.float32)
        else:
            if f.chunks is None:
                x = np.concatenate([np.full(FRAME, stand_in_sample(f.u, j), np.float32) for j in range(f.total)])
                f.chunks = level_limit(x, f.level[0], self.level_ceiling_cdb, chunks=[FRAME] * f.total)
            x = f.chunks[k]
        f.last = x
        return wire_bytes(x, f.enc)

    def fetch_loud(self, n, calls_back=0):
        out = self.loud_out if calls_back == 0 else self.loud_prev
        return [out[b] if out is not None and b < len(out) else np.zeros(0, np.float64) for b in range(n)]

    def fetch_align(self, n, calls_back=0):
        out = self.align_out if calls_back == 0 else self.align_prev
        return [out[b] if out is not None and b < len(out) else np.zeros(0, np.float32) for b in range(n)]

    def fetch_wire(self, n, calls_back=0):
        out = self.wire_out if calls_back == 0 else self.wire_prev
        return [out[b] if out is not None and b < len(out) else b"" for b in range(n)]

    def close(self):
        pass


def _listen_socket(host: str, port: int, reuse_port: bool = True):
    """A listening TCP socket with SO_REUSEPORT: every per-GPU worker process binds the same port
    and the kernel spreads incoming connections over them (no proxy process in the data path)."""
    import socket

    # proto IPPROTO_TCP explicitly: asyncio sets TCP_NODELAY only on transports whose socket says
    # so (proto 0 left Nagle on: every chunk written behind the response headers waited for the
    # client's delayed ACK, ~20 ms on a stream's first chunk); the listener's NODELAY is inherited
    so = socket.socket(socket.AF_INET, socket.SOCK_STREAM, socket.IPPROTO_TCP)
    so.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
    so.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    if reuse_port:
        so.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEPORT, 1)
    so.bind((host, port))
    so.listen(1024)
    return so


def _worker_engine(args, Engine):
    """This process's engine. Under torch.distributed (one rank per GPU): rank 0 packs the weights
    (checkpoint or synthetic) into its engine-owned blob, ONE broadcast over RCCL (xGMI) copies it
    to every rank at load time, the other ranks finalize from it (no per-step
    collective). Returns (engine, rank, world, blob checksum)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    kw = dict(max_slots=args.slots, max_ctx=args.max_ctx, weights_path=args.weights, pipeline=True,
              back_frames=args.back_frames, lsd_decode_steps=args.lsd_steps, max_lsd_steps=args.max_lsd_steps,
              wire=args.wire, tempo=args.wire and args.tempo, flac=args.wire and args.flac,
              pitch=args.wire and args.tempo and args.pitch)
    # (an engine without the stage is created exactly as before; the launcher's stand-in has no wire surface)
    if args.wire and args.volume and Engine is not StandInEngine:
        kw.update(level=True, level_ceiling_db=args.limiter_ceiling_db)
    if args.wire and args.loudness and Engine is not StandInEngine:  # off by default
        kw.update(loud=True)
    if args.align:  # off by default: the engine is created exactly as before
        kw.update(align=True, align_layer=args.align_layer, align_heads=int(str(args.align_heads), 0))
    if Engine is StandInEngine:
        kw["step_s"] = args.stand_in_step_ms / 1000.0
    if "WORLD_SIZE" not in os.environ:  # a plain single-GPU server
        return Engine(device=local, **kw), 0, 1, None
    import torch
    import torch.distributed as dist

    stand_in = Engine is StandInEngine
    if not stand_in:
        torch.cuda.set_device(local)
    dist.init_process_group("gloo" if stand_in else "nccl")
    dev = "cpu" if stand_in else f"cuda:{local}"
    blob = torch.empty(Engine.weight_blob_bytes() // 4, dtype=torch.float32, device=dev)
    if stand_in and rank == 0:
        blob.copy_(torch.arange(blob.numel(), dtype=torch.float32))
    eng = Engine(device=local, weight_blob=blob.data_ptr(), defer_weights=rank != 0, **kw)
    if not stand_in:
        torch.cuda.synchronize()
    dist.broadcast(blob, src=0)
    if not stand_in:
        torch.cuda.synchronize()
    if rank != 0:
        eng.finalize()
    checksum = float(blob[:1024].double().sum().item())
    dist.barrier()
    return eng, rank, world, checksum


def main(argv=None):
    """python -m pocket_tts_amd.serve --voice NAME=prompt.npy [--voice ...] [--tokenizer t.json]
    [--gpus N] [--slots 32] [--port 8000]

    --gpus N > 1: one worker PROCESS per GPU (launched as N ranks of torch.distributed.run, a
    child process; this parent never touches the GPU), each with its own engine, scheduler and
    HTTP server on the same SO_REUSEPORT port: no shared GIL, no proxy hop; the weights are packed
    once and broadcast over RCCL at load time."""
    import argparse

    # before any HIP initialization (a torchrun worker's RCCL setup comes before the engine library
    # loads, which sets the same default): graph kernel nodes instead of captured packets (capi.cpp)
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

    ap = argparse.ArgumentParser()
    ap.add_argument("--voice", action="append", default=[], help="NAME=path (.npy prompt [F,1024] or .wav)")
    ap.add_argument("--tokenizer", default=None)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--torchrun", action="store_true",
                    help="launch the worker(s) as torch.distributed ranks even for --gpus 1 (the N-GPU path)")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--max-ctx", type=int, default=1024)
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--back-frames", type=int, default=2, choices=(1, 2, 4, 8),
                    help="frames per Mimi decode pass (ptts_engine_config.back_frames): 2, the throughput "
                         "configuration bench.py measures (two more calls of frame lag, ~1.2 ms at B = 32)")
    ap.add_argument("--lsd-steps", type=int, default=1,
                    help="LSD Euler steps of a request that names none (TTSModel.lsd_decode_steps)")
    ap.add_argument("--max-lsd-steps", type=int, default=None,
                    help="largest per-request lsd_steps (the engine's cap; default: --lsd-steps). Requests with "
                         "different counts share the batch; a step costs the largest count among its open rows")
    ap.add_argument("--wire", action=argparse.BooleanOptionalAction, default=True,
                    help="wire formats converted on the GPU (requests' sample_rate / encoding); --no-wire: the "
                         "engine as before, such requests get 400")
    ap.add_argument("--flac", action=argparse.BooleanOptionalAction, default=True,
                    help="FLAC output (requests' encoding / response_format flac) encoded on the GPU; needs --wire (off "
                         "with --no-wire); --no-flac: the wire-enabled engine as before, such requests get 400")
    ap.add_argument("--tempo", action=argparse.BooleanOptionalAction, default=True,
                    help="per-request speech speed (requests' speed) time-scaled on the GPU; needs --wire (off "
                         "with --no-wire); --no-tempo: the wire-enabled engine as before, such requests get 400")
    ap.add_argument("--pitch", action=argparse.BooleanOptionalAction, default=True,
                    help="per-request pitch (requests' pitch, semitones) shifted on the GPU; needs --tempo (off with "
                         "--no-tempo or --no-wire); --no-pitch: the tempo-enabled engine as before, such requests get 400")
    ap.add_argument("--volume", action=argparse.BooleanOptionalAction, default=True,
                    help="per-request volume (requests' volume_db and limit): gain and a look-ahead peak limiter on the "
                         "GPU; needs --wire (off with --no-wire); --no-volume: the engine as before, such requests get 400")
    ap.add_argument("--limiter-ceiling-db", type=float, default=-1.0,
                    help="the level stage's ceiling in dBFS, -40 .. 0: no sample of a row with volume_db or limit "
                         "leaves it")
    ap.add_argument("--loudness", action=argparse.BooleanOptionalAction, default=False,
                    help="loudness (requests' `loudness` and `loudness_lufs`; GET /voices/NAME): a BS.1770 meter on the "
                         "GPU, every registered voice calibrated on a fixed sentence; needs --wire, and --volume for "
                         "`loudness_lufs`; off by default: the engine as before, such requests get 400")
    ap.add_argument("--align", action=argparse.BooleanOptionalAction, default=False,
                    help="word timestamps (requests' `timestamps` on /generate and /v1/audio/speech): one more launch in "
                         "the FlowLM step delivers a text-attention row per frame; off by default (which layer and "
                         "heads align is a property of the checkpoint: tools/align_heads.py)")
    ap.add_argument("--align-layer", type=int, default=0, help="the FlowLM layer (0 .. 5) the align stage reads")
    ap.add_argument("--align-heads", default="0xFFFF",
                    help="bit mask of the heads (bit h = head h of 16) the align stage averages")
    ap.add_argument("--long-form", action=argparse.BooleanOptionalAction, default=False,
                    help="default of requests that do not say `long_form`: split the text into pause and sentence "
                         "segments (the reference's generate_stream_long) and run them on parallel rows")
    ap.add_argument("--continuity", action=argparse.BooleanOptionalAction, default=False,
                    help="default of requests that do not say `continuity`: the long-form cut, each sentence chunk "
                         "teacher-forced through the one before it and decoded on from its codec state")
    ap.add_argument("--segment-rows", type=int, default=4,
                    help="text segments of one long-form request that may be waiting or active at once "
                         "(clamped to --slots)")
    ap.add_argument("--preview-rows", type=int, default=8,
                    help="first-frame previews: rows per call whose first frame is decoded at once (0: off)")
    ap.add_argument("--voice-cache", type=int, default=64,
                    help="per-request voices (base64 WAV in the `voice` field) kept per engine, least recently used out")
    ap.add_argument("--max-voice-seconds", type=float, default=30.0,
                    help="longest voice clip a request or POST /voices may bring (also sizes the clone workspace)")
    ap.add_argument("--stand-in-engine", action="store_true",
                    help="CPU self-test of the launcher and routing: a stand-in engine that computes nothing")
    ap.add_argument("--stand-in-step-ms", type=float, default=0.0, help="--stand-in-engine: time per step")
    ap.add_argument("--no-redirect", action="store_true",
                    help="multi-process server: no overflow redirect to the least-loaded worker (LoadBoard)")
    args = ap.parse_args(argv)
    import sys

    if (args.gpus > 1 or args.torchrun) and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess

        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            mport = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", f"--master-port={mport}", "-m", "pocket_tts_amd.serve",
               *(argv if argv is not None else sys.argv[1:])]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0",
                   PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(__file__)),
                                               os.environ.get("PYTHONPATH", "")]))
        sys.exit(subprocess.run(cmd, env=env).returncode)
    # the scheduler thread drops the GIL in every engine call; with the default 5 ms switch
    # interval it can wait that long to get it back from the HTTP threads (one engine step is
    # < 1 ms), so hand the GIL over sooner
    sys.setswitchinterval(2e-4)
    if args.stand_in_engine:
        Engine = StandInEngine
    else:
        from .engine import Engine
    engine, rank, world, checksum = _worker_engine(args, Engine)
    voices: dict[str, Voice] = {}
    for spec in args.voice or []:
        name, path = spec.split("=", 1)
        if path.endswith(".npy"):
            voices[name] = engine.voice_from_prompt(np.load(path, allow_pickle=False).astype(np.float32))
        else:  # a WAV voice prompt: resampled to 24 kHz on the GPU, Mimi-encoded (tts_model.rs:446-463)
            from .audio import read_wav

            audio, sr = read_wav(path)
            if audio.shape[0] != 1:
                raise SystemExit(f"voice prompt {path} must be mono")
            voices[name] = engine.voice_from_audio(audio[0], sr)
    if not voices:
        raise SystemExit("at least one --voice NAME=path is required")
    # the clone workspace of per-request voices, sized once for the longest clip accepted
    engine.reserve_voice_jobs(max(1, min(args.max_ctx - 1, math.ceil(args.max_voice_seconds * SAMPLE_RATE / FRAME) + 1)))
    scheduler = BatchScheduler(engine, preview_rows=args.preview_rows, voice_cache=args.voice_cache,
                               segment_rows=args.segment_rows)
    service = TTSService(scheduler, voices, default_voice=next(iter(voices)),
                         tokenizer=load_tokenizer(args.tokenizer) if args.tokenizer else None,
                         lsd_decode_steps=args.lsd_steps, max_lsd_steps=args.max_lsd_steps,
                         max_voice_seconds=args.max_voice_seconds, long_form=args.long_form,
                         continuity=args.continuity)
    service.worker = {"rank": rank, "world": world, "pid": os.getpid(), "weights_checksum": checksum}
    socks = [_listen_socket(args.host, args.port)]
    board = None
    if world > 1 and not args.no_redirect:  # least-loaded dispatch across the workers (LoadBoard)
        board = LoadBoard(args.port, world, rank, scheduler.max_rows)
        board.publish(0)
        priv = _listen_socket(args.host, 0, reuse_port=False)
        board.set_private_port(priv.getsockname()[1])
        socks.append(priv)
        scheduler.on_load = board.publish
        service.board, service.shared_port = board, args.port
    import uvicorn

    app = create_app(service)
    try:
        uvicorn.Server(uvicorn.Config(app, log_level="warning")).run(sockets=socks)
    finally:
        if board is not None:
            board.close(unlink=rank == 0)


if __name__ == "__main__":
    main()
