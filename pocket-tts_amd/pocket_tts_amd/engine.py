"""Batched engine over the C ABI: one engine per GPU, `max_slots` concurrent utterances."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import (BACK_BF16, BACK_F32, BACK_F32X6, DIM, F32P, FRAME, I32P, LDIM, SAMPLES_F32, SAMPLES_S16, U8P,
                   WIRE_ALAW, WIRE_FLAC, WIRE_CHUNK_MAX, WIRE_CHUNK_MAX_LEVEL, WIRE_CHUNK_MAX_TEMPO, WIRE_NONE, WIRE_RATES, WIRE_S16, WIRE_ULAW, EngineConfig, GenParams,
                   SAMPLE_RATE, SlotOpts5, SlotOpts6, ALIGN_TOKENS, check, fptr, lib, u8ptr)
from .audio import ENCODINGS, level_cdb, pitch_cents, pitch_plan, speed_permille

# wire encodings by the names the server's `encoding` field uses (PTTS_WIRE_*)
WIRE_ENCODINGS = {"pcm_s16le": WIRE_S16, "ulaw": WIRE_ULAW, "alaw": WIRE_ALAW, "flac": WIRE_FLAC}


def wire_encoding_code(encoding) -> int:
    """PTTS_WIRE_* of an encoding given by name (WIRE_ENCODINGS), by code, or None (WIRE_NONE)."""
    if encoding is None:
        return WIRE_NONE
    if isinstance(encoding, str):
        if encoding not in WIRE_ENCODINGS:
            raise ValueError(f"encoding must be one of {sorted(WIRE_ENCODINGS)}, got {encoding!r}")
        return WIRE_ENCODINGS[encoding]
    return int(encoding)


@dataclass
class GenerationParams:
    """Per-utterance knobs; field meaning follows TTSModel (tts_model.rs:22-49, 968-969)."""

    temp: float = 0.7
    eos_threshold: float = -4.0
    noise_clamp: float | None = None
    frames_after_eos: int = 3
    max_frames: int = 250
    seed: int = 0
    # the utterance's own LSD Euler step count (TTSModel.lsd_decode_steps, the server's lsd_steps),
    # 1 .. the engine's cap; None: the engine's lsd_decode_steps. Not part of ptts_gen_params: the
    # admission passes it beside the struct (ptts_slot_opts.lsd_steps).
    lsd_steps: int | None = None
    # wire format of the row (wire-enabled engines; Engine.fetch_wire returns its bytes): sample_rate
    # one of WIRE_RATES, encoding "pcm_s16le" / "ulaw" / "alaw" / "flac" (or a PTTS_WIRE_* code). None in both:
    # no wire output; None in one: 24000 / 16-bit. Passed beside the struct too (ptts_slots_open_opts).
    sample_rate: int | None = None
    encoding: str | int | None = None
    # speech speed of the row's wire bytes (tempo-enabled engines), 0.5 .. 2.0; None or 1.0: unchanged.
    # A speed with no wire format implies 24000 / 16-bit. The f32 PCM of fetch() never depends on it.
    speed: float | None = None
    # pitch shift of the row's wire bytes in semitones (pitch-enabled engines), -12 .. 12; None or 0:
    # unchanged. A resampling shift (formants move too) at the duration `speed` asks for (DESIGN.md
    # section 23). A pitch with no wire format implies 24000 / 16-bit; fetch()'s f32 PCM never depends on it.
    pitch: float | None = None
    # volume of the row's wire bytes in dB (level-enabled engines), -24 .. 24, and `limit`: run the
    # row through the look-ahead peak limiter (the engine's ceiling) even with no gain. A row with a
    # gain always runs through it. None / 0 and False: unchanged. Either with
    # no wire format implies 24000 / 16-bit; fetch()'s f32 PCM never depends on them.
    volume_db: float | None = None
    limit: bool = False
    # latent prefix and codec continuity (ptts_slot_opts.prefix_latents / .keep_codec; DESIGN.md
    # section 20): the row starts as if it had been teacher-forced through these [n, 32] FlowLM
    # latents (values fetch() returned), and with keep_codec on the codec state its slot ended on.
    prefix_latents: np.ndarray | None = None
    keep_codec: bool = False
    # word alignment (align-enabled engines): every frame of the row also
    # carries the attention its FlowLM step paid to the row's text tokens (Engine.fetch_align). At
    # most ALIGN_TOKENS token ids. No other output of the row depends on it.
    align: bool = False
    # loudness meter (loudness-enabled engines): every frame of the row also
    # carries the K-weighted energies of the 100 ms sub-blocks it completed (Engine.fetch_loud),
    # measured on the signal the wire stage reads. With no wire format it implies 24000 / 16-bit.
    # No other output of the row depends on it.
    loudness: bool = False

    def prefix(self) -> np.ndarray | None:
        """The prefix as a contiguous [n, 32] float32 array; None: no prefix."""
        if self.prefix_latents is None:
            return None
        a = np.ascontiguousarray(self.prefix_latents, np.float32)
        if a.ndim != 2 or a.shape[1] != LDIM:
            raise ValueError(f"prefix_latents must be [n, {LDIM}], got {a.shape}")
        return a if a.shape[0] else None

    def output(self) -> "OutputOptions":
        """The six output fields as they stand (not normalised: Engine callers may set any value)."""
        return OutputOptions(self.sample_rate, self.encoding, self.speed, self.pitch, self.volume_db, self.limit)

    def wire(self) -> tuple[int, int]:
        """(wire_rate, wire_encoding) of ptts_slot_opts; (0, 0): none."""
        return self.output().codes()[:2]

    def opts(self) -> tuple[int, int, int]:
        """(wire_rate, wire_encoding, speed_permille) of ptts_slot_opts; all 0: the defaults."""
        return self.output().codes()[:3]

    def cents(self) -> int:
        """pitch_cents of ptts_slot_opts; 0: none."""
        return self.output().codes()[3]

    def level(self) -> tuple[int, int]:
        """(gain_cdb, limit) of ptts_slot_opts; (0, 0): the row is not in the level stage."""
        return self.output().codes()[4:]

    def slot_opts(self, default_lsd: int = 0, metered: bool | None = None) -> SlotOpts5 | SlotOpts6:
        """The row's ptts_slot_opts, the whole 64-byte struct (fields it does not name are 0), or the
        72-byte struct for a metered row (metered=True: that struct whatever the row asks).
        default_lsd: lsd_steps of a row that names none (0: the engine's cap). The struct keeps the
        prefix array it points into alive."""
        K = SlotOpts6 if (self.loudness if metered is None else metered) else SlotOpts5
        o = K(size=C.sizeof(K), lsd_steps=int(default_lsd if self.lsd_steps is None else self.lsd_steps))
        if K is SlotOpts6:
            o.loud = int(bool(self.loudness))
        o.wire_rate, o.wire_encoding, o.speed_permille, o.pitch_cents, o.gain_cdb, o.limit = self.output().codes()
        o.keep_codec, o.align = int(self.keep_codec), int(bool(self.align))
        pre = o._prefix = self.prefix()
        if pre is not None:
            o.prefix_latents, o.n_prefix = pre.ctypes.data, pre.shape[0]
        return o

    def to_c(self) -> GenParams:
        return GenParams(float(self.temp), float(self.eos_threshold),
                         float(self.noise_clamp) if self.noise_clamp is not None else 0.0,
                         int(self.frames_after_eos), int(self.max_frames), int(self.seed) & (2**64 - 1))


@dataclass(frozen=True)
class OutputOptions:
    """What a request asks of its row's audio output, the fields of the same names of
    GenerationParams: the one place that says what they come to. of() is the way in from a caller's
    raw values; a value it returns holds None / False in every field that changes nothing."""

    sample_rate: int | None = None
    encoding: str | int | None = None
    speed: float | None = None
    pitch: float | None = None
    volume_db: float | None = None
    limit: bool = False

    @classmethod
    def of(cls, sample_rate=None, encoding=None, speed=None, pitch=None, volume_db=None, limit=None):
        """Normalised: speed 1.0 is no speed, pitch 0 no pitch, volume 0 without limit no level (else
        rounded to hundredths of a dB). ValueError for a value out of range, or a pitch that with
        this speed leaves the time-scaling range."""
        speed = float(speed) if speed_permille(speed) else None
        pitch = float(pitch) if pitch_cents(pitch) else None
        if pitch is not None:
            pitch_plan(pitch_cents(pitch), speed_permille(speed))
        cdb = level_cdb(volume_db)
        volume_db = cdb / 100.0 if cdb or limit else None
        return cls(sample_rate, encoding, speed, pitch, volume_db, bool(limit) and volume_db is not None)

    def codes(self) -> tuple[int, int, int, int, int, int]:
        """(wire_rate, wire_encoding, speed_permille, pitch_cents, gain_cdb, limit) of ptts_slot_opts,
        0 for none. Values out of range are passed on as they are, rounded: the admission refuses them."""
        sp = 0 if self.speed is None else round(float(self.speed) * 1000)
        return (int(self.sample_rate or 0), wire_encoding_code(self.encoding), 0 if sp == 1000 else sp,
                0 if self.pitch is None else round(100.0 * float(self.pitch)),
                0 if self.volume_db is None else round(100.0 * float(self.volume_db)), int(self.limit or 0))

    @property
    def wire(self) -> tuple[int, str] | None:
        """(rate, encoding name) of a wire row, whose items are bytes the engine converted: a row
        with any of the options, at 24000 / pcm_s16le unless it says otherwise (the engine's rule,
        Engine::slots_open). None: f32 frames."""
        c = self.codes()
        return (c[0] or SAMPLE_RATE, ENCODINGS[(c[1] or WIRE_S16) - 1]) if any(c) else None

    def apply(self, p: GenerationParams) -> GenerationParams:
        p.sample_rate, p.encoding, p.speed, p.pitch = self.sample_rate, self.encoding, self.speed, self.pitch
        p.volume_db, p.limit = self.volume_db, self.limit
        return p


class Voice:
    """Immutable FlowLM KV prefix of a voice prompt (the reference's ModelState)."""

    def __init__(self, engine: "Engine", handle: int):
        self._engine = engine
        self.handle = C.c_void_p(handle)

    @property
    def n_frames(self) -> int:
        return lib().ptts_voice_len(self.handle)

    def conditioning(self) -> np.ndarray:
        out = np.zeros((self.n_frames, DIM), np.float32)
        check(lib().ptts_voice_conditioning(self.handle, fptr(out), out.shape[0]))
        return out

    def ready(self, wait: bool = False) -> bool:
        """The voice's job has run (ptts_voice_ready); always True for a synchronously made voice.
        wait=True blocks until it has. Admission never needs this: it is ordered on the GPU."""
        r = C.c_int(0)
        check(lib().ptts_voice_ready(self.handle, int(wait), C.byref(r)))
        return bool(r.value)

    def close(self):
        """Destroy the voice (waits for a pending job of it; slots still reading it keep it alive)."""
        if self.handle:
            lib().ptts_voice_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class StepResult:
    pcm: np.ndarray  # [n_rows, 1920]
    valid: np.ndarray  # [n_rows] bool, row produced a frame this step
    last: np.ndarray  # [n_rows] bool, that frame was the row's final one
    eos_logits: np.ndarray  # [n_rows]
    latents: np.ndarray  # [n_rows, 32]


RESAMPLERS = {"poly": 0, "rubato": 1}  # PTTS_RESAMPLE_POLY, PTTS_RESAMPLE_RUBATO_SEPTIC


def resampler_code(name: str) -> int:
    if name not in RESAMPLERS:
        raise ValueError(f"resampler must be one of {sorted(RESAMPLERS)}, got {name!r}")
    return RESAMPLERS[name]


class Engine:
    def __init__(self, device: int = 0, max_slots: int = 1, max_ctx: int = 1024, lsd_decode_steps: int = 1,
                 seed: int = 0x5EED, weights_path: str | None = None, weight_blob: int | None = None,
                 defer_weights: bool = False, pipeline: bool = False, weight_quant: int = 0, fp8_gemm: bool = False,
                 cfg_yaml: str | None = None, back_frames: int = 1, back_bf16: bool = False,
                 back_mfma: int | None = None, max_lsd_steps: int | None = None, wire: bool = False,
                 tempo: bool = False, flac: bool = False, pitch: bool = False, level: bool = False,
                 level_ceiling_db: float = -1.0, align: bool = False, align_layer: int = 0,
                 align_heads: int = 0xFFFF, loud: bool = False):
        """lsd_decode_steps: the Euler step count of an utterance whose GenerationParams names none.
        max_lsd_steps: the cap on the per-utterance counts (GenerationParams.lsd_steps), the engine's
        ptts_engine_config.lsd_decode_steps; None: lsd_decode_steps itself. Rows with different
        counts share one batched step (lsd_steps()).
        pipeline=True: overlapped stepping, each step() returns the frame produced by the
        previous call (see ptts_engine_config.pipeline). weight_quant: QUANT_NONE / QUANT_FLOW_LM /
        QUANT_ALL, the reference's simulated int8 weight quantization (quantize.rs), with the
        FlowLM step GEMMs streaming int8 codes. fp8_gemm=True: the large FlowLM step GEMMs run as
        fp8 W8A8 MFMA (accuracy-gated; see ptts_engine_config.fp8_gemm). cfg_yaml: the reference's
        model config (config/b6369a24.yaml), checked against the compiled dimensions.
        back_frames=n, 2 or 4 (pipelined only): n frames per Mimi-decode pass; a step() returns the
        frame computed 2 n - 1 calls earlier (`frame_lag`). back_mfma (ptts_engine_config.back_mfma): how the
        Mimi decode's GEMMs and convs use the matrix cores, BACK_F32 (exact f32 FMA chain), BACK_F32X6
        (f32 products as six bf16 piece products, f32 accuracy) or BACK_BF16 (operands rounded to
        bf16: a variant gated on PCM accuracy); back_bf16=True is BACK_BF16.
        wire=True (ptts_wire_enable): rows admitted with GenerationParams.sample_rate / encoding also
        get their wire bytes, converted on the GPU (fetch_wire).
        tempo=True (ptts_tempo_enable; needs wire): rows admitted with GenerationParams.speed have
        their wire bytes time-scaled on the GPU.
        pitch=True (ptts_pitch_enable; needs tempo): rows admitted with GenerationParams.pitch have
        their wire bytes shifted in pitch on the GPU.
        level=True (ptts_level_enable; needs wire): rows admitted with GenerationParams.volume_db or
        .limit have their wire bytes scaled and peak-limited to level_ceiling_db (dBFS, -40 .. 0) on
        the GPU.
        flac=True (ptts_flac_enable; needs wire): rows admitted with encoding "flac" get FLAC frames
        of their 16-bit chunks, encoded on the GPU.
        align=True (ptts_align_enable): rows admitted with GenerationParams.align get, with every
        frame, their step's text-attention row of FlowLM layer align_layer (0 .. 5), averaged over
        the heads of the bit mask align_heads (fetch_align).
        loud=True (ptts_loud_enable; needs wire): rows admitted with GenerationParams.loudness get, with
        every frame, the K-weighted energies of the 100 ms sub-blocks of their output that the frame
        completed (fetch_loud)."""
        if back_mfma is None:
            back_mfma = BACK_BF16 if back_bf16 else BACK_F32
        elif back_bf16 and back_mfma != BACK_BF16:
            raise ValueError("back_bf16=True contradicts back_mfma=%d (pass one of them)" % back_mfma)
        cap = int(lsd_decode_steps if max_lsd_steps is None else max_lsd_steps)
        if not 1 <= int(lsd_decode_steps) <= cap:
            raise ValueError(f"lsd_decode_steps {lsd_decode_steps} outside [1, max_lsd_steps = {cap}]")
        cfg = EngineConfig(device, max_slots, max_ctx, cap, seed,
                           weights_path.encode() if weights_path else None,
                           weight_blob or None, int(defer_weights), int(pipeline), int(weight_quant),
                           int(fp8_gemm), cfg_yaml.encode() if cfg_yaml else None, int(back_frames),
                           int(back_mfma))
        h = C.c_void_p()
        check(lib().ptts_engine_create(C.byref(cfg), C.byref(h)))
        self.handle = h
        self.weight_quant = int(weight_quant)
        self.max_slots = max_slots
        self.max_ctx = max_ctx
        self.lsd_decode_steps = int(lsd_decode_steps)
        self.max_lsd_steps = cap
        self.pipeline = bool(pipeline)
        self.back_frames = int(back_frames) if pipeline else 1
        self.back_mfma = int(back_mfma)
        self.back_bf16 = self.back_mfma == BACK_BF16
        self.wire = bool(wire)
        if wire:
            try:
                check(lib().ptts_wire_enable(self.handle, 1))
            except Exception:
                self.close()
                raise
        self.tempo_enabled = bool(tempo)
        if tempo:
            try:
                check(lib().ptts_tempo_enable(self.handle, 1))
            except Exception:
                self.close()
                raise
        self.pitch_enabled = bool(pitch)
        if pitch:
            try:
                check(lib().ptts_pitch_enable(self.handle, 1))
            except Exception:
                self.close()
                raise
        self.flac_enabled = bool(flac)
        if flac:
            try:
                check(lib().ptts_flac_enable(self.handle, 1))
            except Exception:
                self.close()
                raise
        self.level_enabled = bool(level)
        self.level_ceiling_cdb = 0
        if level:
            try:
                self.level_ceiling_cdb = level_cdb(level_ceiling_db, -40.0, 0.0, "level_ceiling_db")
                check(lib().ptts_level_enable(self.handle, 1, self.level_ceiling_cdb))
            except Exception:
                self.close()
                raise
        self.align_enabled = bool(align)
        self.align_layer, self.align_heads = int(align_layer), int(align_heads)
        if align:
            try:
                check(lib().ptts_align_enable(self.handle, 1, self.align_layer, self.align_heads & 0xFFFFFFFF))
            except Exception:
                self.close()
                raise
        self._align_buf = self._align_n = None
        self.loud_enabled = bool(loud)
        if loud:
            try:
                check(lib().ptts_loud_enable(self.handle, 1))
            except Exception:
                self.close()
                raise
        self.wire_chunk_max = WIRE_CHUNK_MAX_LEVEL if level else WIRE_CHUNK_MAX_TEMPO if tempo else WIRE_CHUNK_MAX
        self._wire_buf = self._wire_n = None

    def test_gemm(self, layout: int, x: np.ndarray, w: np.ndarray, splits: int = 1, tail_slices: int = 0) -> np.ndarray:
        """GEMM-core test hook (ptts_test_gemm): x [m][k] @ w [n][k]^T on tile `layout`; splits > 1
        returns the [splits][m][n] partial slabs."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        m, k = x.shape
        n = w.shape[0]
        y = np.empty((splits, m, n) if splits > 1 else (m, n), np.float32)
        check(lib().ptts_test_gemm(self.handle, layout, m, n, k, splits, tail_slices, fptr(x), fptr(w), fptr(y)))
        return y

    def test_attention(self, kind: int, qkv: np.ndarray, kv: np.ndarray, window: int = 0, *, slot0: int = 0,
                       rps: int = 16, p0: int = 0, pos=None, tab=None, ptab=None, pre=None):
        """Attention-path test hook (ptts_test_attention). kind 0: qkv_rope_append + attention(qg = 16),
        1: the fused Mimi step attention16_qkv, 2: attention_step_qkv. qkv [m][3 nh 64] dense rows or
        [S][m][3 nh 64] partial slabs; kv [slots][2][nh][cap][64], the store before the call; rows map
        to (slot, position) by slot0 / rps / p0 / pos [slots] or by the table tab (with ptab: the
        compact form, tab the tokens and ptab the padded 16-row groups); pre: one [2][nh][F][64]
        prefix (or None) per slot. Returns (o, kv_after, q): q the rotated queries for kind 0, else
        None."""
        qkv = np.ascontiguousarray(qkv, np.float32)
        kv_out = np.array(kv, np.float32, order="C")  # a copy: the call writes it
        slots, two, nh, cap, hd = kv_out.shape
        splits, m = (qkv.shape[0], qkv.shape[1]) if qkv.ndim == 3 else (0, qkv.shape[0])
        if two != 2 or hd != 64 or qkv.shape[-1] != 3 * nh * 64:
            raise ValueError("test_attention: qkv / kv shapes disagree")

        def iarr(a, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.int32)
            if a.shape != (n,):
                raise ValueError(f"test_attention: expected {n} ints, got shape {a.shape}")
            return a

        def iptr(a):
            return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))

        pos, tab = iarr(pos, slots), iarr(tab, m)
        mpad = 0 if ptab is None else len(ptab)
        ptab = iarr(ptab, mpad)
        pre_cat = pre_len = None
        if pre is not None:
            if len(pre) != slots:
                raise ValueError("test_attention: one prefix (or None) per slot")
            parts = [np.zeros((2, nh, 0, 64), np.float32) if p is None else np.ascontiguousarray(p, np.float32)
                     for p in pre]
            if any(p.ndim != 4 or p.shape[:2] != (2, nh) or p.shape[3] != 64 for p in parts):
                raise ValueError("test_attention: a prefix is [2][nh][F][64]")
            pre_len = np.array([p.shape[2] for p in parts], np.int32)
            pre_cat = np.concatenate([p.ravel() for p in parts] + [np.zeros(4, np.float32)])
        q = np.zeros((mpad if ptab is not None else m, nh * 64), np.float32) if kind == 0 else None
        o = np.zeros((m, nh * 64), np.float32)
        check(lib().ptts_test_attention(self.handle, kind, m, nh, cap, window, slots, splits, fptr(qkv), fptr(kv_out),
                                        fptr(pre_cat), iptr(pre_len), slot0, rps, p0, iptr(pos), iptr(tab), iptr(ptab),
                                        mpad, fptr(q), fptr(o)))
        return o, kv_out, q

    def test_align(self, qkv: np.ndarray, kv: np.ndarray, pos, tab, head_mask: int, out: np.ndarray, pre=None):
        """Align test hook (ptts_test_align): the product launcher on host operands, row r = slot r.
        qkv [m][3 nh 64] dense rows or [S][m][3 nh 64] slabs; kv [m][2][nh][cap][64]; pos [m]; tab
        [m][2] = {t0, n}; out [m][1 + ALIGN_TOKENS] float32 words going in (sentinels). Returns
        (counts [m] int32, rows [m][ALIGN_TOKENS] float32) as the call left them."""
        qkv = np.ascontiguousarray(qkv, np.float32)
        kv = np.ascontiguousarray(kv, np.float32)
        m, two, nh, cap, hd = kv.shape
        splits = qkv.shape[0] if qkv.ndim == 3 else 0
        if two != 2 or hd != 64 or qkv.shape[-1] != 3 * nh * 64 or qkv.shape[-2] != m:
            raise ValueError("test_align: qkv / kv shapes disagree")
        pos = np.ascontiguousarray(pos, np.int32).reshape(m)
        tab = np.ascontiguousarray(tab, np.int32).reshape(m, 2)
        o = np.array(out, np.float32, order="C").reshape(m, 1 + ALIGN_TOKENS)
        pre_cat = pre_len = None
        if pre is not None:
            parts = [np.zeros((2, nh, 0, 64), np.float32) if p is None else np.ascontiguousarray(p, np.float32)
                     for p in pre]
            pre_len = np.array([p.shape[2] for p in parts], np.int32)
            pre_cat = np.concatenate([p.ravel() for p in parts] + [np.zeros(4, np.float32)])
        i32 = C.POINTER(C.c_int32)
        # declared in csrc/test_hooks.h, not in the headers whose symbols _lib.SIGNATURES mirrors: bound here
        fn = lib().ptts_test_align
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 4 + [F32P] * 3 + [i32] * 3 + [C.c_uint, F32P]
        check(fn(self.handle, m, nh, cap, splits, fptr(qkv), fptr(kv), fptr(pre_cat),
                                    None if pre_len is None else pre_len.ctypes.data_as(i32), pos.ctypes.data_as(i32),
                                    tab.ctypes.data_as(i32), int(head_mask) & 0xFFFFFFFF, fptr(o)))
        return o[:, 0].copy().view(np.int32), o[:, 1:].copy()

    def test_row_reduce(self, p: np.ndarray, *, bias=None, gate=None, r=None, act: int = 0, ln: bool = False,
                        eps: float = 1e-5, ln_w=None, ln_b=None, mscale=None, mshift=None, hfrag: bool = False,
                        front: bool = False):
        """Row-reduce test hook (ptts_test_row_reduce): the product launcher on p [S][m][n] with the
        optional operands bias [n], gate / r [m][n], LayerNorm (ln_w, ln_b [n]) and modulate (mscale,
        mshift [m][n]); act 0 none, 1 GELU. Returns (y, h, hfrag): h None without ln, hfrag (the
        [32][1024] A-fragment copy of h) None unless asked for."""
        p = np.ascontiguousarray(p, np.float32)
        s, m, n = p.shape

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32)
            if a.shape != shape:
                raise ValueError(f"test_row_reduce: expected shape {shape}, got {a.shape}")
            return a

        bias, ln_w, ln_b = arr(bias, (n,)), arr(ln_w, (n,)), arr(ln_b, (n,))
        gate, r, mscale, mshift = (arr(a, (m, n)) for a in (gate, r, mscale, mshift))
        y = np.empty((m, n), np.float32)
        h = np.empty((m, n), np.float32) if ln else None
        hf = np.empty(32 * 1024, np.float32) if hfrag else None
        # declared in csrc/test_hooks.h, not in the headers whose symbols _lib.SIGNATURES mirrors: bound here
        fn = lib().ptts_test_row_reduce
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_int] + [F32P] * 11
        check(fn(self.handle, m, n, s, act, int(ln), eps, int(front), fptr(p), fptr(bias), fptr(gate), fptr(r),
                 fptr(ln_w), fptr(ln_b), fptr(mscale), fptr(mshift), fptr(y), fptr(h), fptr(hf)))
        return y, h, hf

    def lsd_steps(self) -> tuple[int, int]:
        """(cap, last_run): the cap on the per-utterance Euler step counts, and the steps the most
        recent step call ran: the largest count among its rows still open (ptts_lsd_steps)."""
        cap, run = C.c_int(0), C.c_int(0)
        check(lib().ptts_lsd_steps(self.handle, C.byref(cap), C.byref(run)))
        return int(cap.value), int(run.value)

    def _row_lsd(self, params: GenerationParams) -> int:
        return int(self.lsd_decode_steps if params.lsd_steps is None else params.lsd_steps)

    def frame_lag(self) -> tuple[int, int]:
        """(lag, admit_delay): a frame arrives `lag` calls after the call that computed it; the
        rows of the latest admission start `admit_delay` calls late (ptts_frame_lag)."""
        d = C.c_int(0)
        lag = int(lib().ptts_frame_lag(self.handle, C.byref(d)))
        return lag, int(d.value)

    @staticmethod
    def check_config(cfg_yaml: str) -> None:
        """Raise PocketTTSError unless the reference model config at `cfg_yaml` states the
        dimensions this build implements (b6369a24); no GPU needed (ptts_config_check)."""
        check(lib().ptts_config_check(cfg_yaml.encode()))

    @staticmethod
    def gemm_tiles() -> list[dict]:
        """The GEMM tiles of the loaded library (ptts_gemm_tiles; no GPU needed): id, tile m x n, bk,
        operands ("f32" | "bf16" | "bf16x6") and whether test_gemm's tail_slices is served."""
        buf = C.create_string_buffer(1 << 14)
        check(lib().ptts_gemm_tiles(buf, len(buf)))
        out = []
        for line in buf.value.decode().splitlines():
            i, tm, tn, bk, ops, tail = line.split("\t")
            out.append({"id": int(i), "tm": int(tm), "tn": int(tn), "bk": int(bk), "operands": ops, "tail": tail == "1"})
        return out

    @staticmethod
    def weight_blob_bytes() -> int:
        return int(lib().ptts_weight_blob_bytes())

    @staticmethod
    def pack_weights(seed: int = 0x5EED, weights_path: str | None = None, weight_quant: int = 0) -> np.ndarray:
        """Packed weight blob (engine device layout) built on the host; no GPU needed.
        weight_quant applies the reference's quantize_weights (quantize.rs) while packing."""
        out = np.empty(Engine.weight_blob_bytes() // 4, np.float32)
        check(lib().ptts_pack_weights_ex(seed, weights_path.encode() if weights_path else None, int(weight_quant),
                                         out.ctypes.data_as(F32P), out.nbytes))
        return out

    @staticmethod
    def weight_manifest() -> list[tuple[str, tuple[int, ...]]]:
        """(checkpoint tensor name, shape) of every tensor the weight packer reads (host only)."""
        need = C.c_size_t(0)
        check(lib().ptts_weight_manifest(None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        check(lib().ptts_weight_manifest(buf, need.value, None))
        out = []
        for line in buf.value.decode().splitlines():
            name, dims = line.split("\t")
            out.append((name, tuple(int(x) for x in dims.split(",")) if dims else ()))
        return out

    @property
    def fp8_matrices(self) -> int:
        """FlowLM GEMM weight matrices on the fp8 W8A8 path (0 unless fp8_gemm)."""
        return int(lib().ptts_engine_fp8_matrices(self.handle))

    @property
    def int8_matrices(self) -> int:
        """FlowLM GEMM weight matrices streamed as int8 codes (0 unless weight_quant)."""
        return int(lib().ptts_engine_int8_matrices(self.handle))

    def weight_blob(self) -> int:
        return int(lib().ptts_engine_weight_blob(self.handle) or 0)

    def load_blob(self, blob: np.ndarray):
        """Fill a deferred engine's weights from a host blob (Engine.pack_weights)."""
        blob = np.ascontiguousarray(blob, np.float32)
        check(lib().ptts_engine_load_blob(self.handle, blob.ctypes.data_as(F32P), blob.nbytes))

    def finalize(self):
        check(lib().ptts_engine_finalize(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            lib().ptts_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- voices
    def voice_from_prompt(self, prompt: np.ndarray) -> Voice:
        p = np.ascontiguousarray(prompt, np.float32).reshape(-1, DIM)
        h = C.c_void_p()
        check(lib().ptts_voice_from_prompt(self.handle, fptr(p), p.shape[0], C.byref(h)))
        return Voice(self, h.value)

    def voice_from_pcm(self, pcm: np.ndarray) -> Voice:
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        h = C.c_void_p()
        check(lib().ptts_voice_from_pcm(self.handle, fptr(x), x.size, C.byref(h)))
        return Voice(self, h.value)

    def voice_from_audio(self, samples: np.ndarray, sample_rate: int, chunk_frames: int = 0,
                         resampler: str = "poly") -> Voice:
        """Mono samples at any rate -> GPU resample to 24 kHz -> chunked Mimi encode -> voice.
        chunk_frames: 0 = the reference's adaptive rule, > 0 = that many frames, < 0 = one pass.
        resampler: "poly" (resample_poly, the rule the reference's ref.wav fixture pair was made
        with) or "rubato" (the Rust driver's FastFixedIn / Septic, audio.rs:197-255)."""
        x = np.ascontiguousarray(samples, np.float32).reshape(-1)
        h = C.c_void_p()
        check(lib().ptts_voice_from_audio_ex(self.handle, fptr(x), x.size, int(sample_rate), int(chunk_frames),
                                             resampler_code(resampler), C.byref(h)))
        return Voice(self, h.value)

    # -- voice jobs: the same clones on the engine's voice stream, beside the step pipeline
    def voice_job(self, samples: np.ndarray, sample_rate: int, chunk_frames: int = 0,
                  resampler: str = "poly") -> Voice:
        """voice_from_audio as a job (ptts_voice_job_start): returns at once, the voice can be
        admitted immediately, and the step pipeline is not drained. A mono float32
        or int16 array selects the sample format (int16: v / 32768, converted on the GPU); any
        other dtype is converted to float32 first."""
        x = np.asarray(samples)
        fmt = SAMPLES_S16 if x.dtype == np.int16 else SAMPLES_F32
        x = np.ascontiguousarray(x, np.int16 if fmt == SAMPLES_S16 else np.float32).reshape(-1)
        h = C.c_void_p()
        check(lib().ptts_voice_job_start(self.handle, x.ctypes.data_as(C.c_void_p), x.size, fmt, int(sample_rate),
                                         int(chunk_frames), resampler_code(resampler), C.byref(h)))
        return Voice(self, h.value)

    def voice_job_prompt(self, prompt: np.ndarray) -> Voice:
        """voice_from_prompt as a job (ptts_voice_job_start_prompt)."""
        p = np.ascontiguousarray(prompt, np.float32).reshape(-1, DIM)
        h = C.c_void_p()
        check(lib().ptts_voice_job_start_prompt(self.handle, fptr(p), p.shape[0], C.byref(h)))
        return Voice(self, h.value)

    def reserve_voice_jobs(self, max_frames: int):
        """Pre-size the voice workspace for clips of up to max_frames frames (ptts_voice_jobs_reserve)."""
        check(lib().ptts_voice_jobs_reserve(self.handle, int(max_frames)))

    def resample(self, x: np.ndarray, sr_from: int, sr_to: int = 24000, resampler: str = "poly") -> np.ndarray:
        """The GPU resampler on its own (ptts_resample_ex)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        code = resampler_code(resampler)
        n = lib().ptts_resample_len_ex(x.size, int(sr_from), int(sr_to), code)
        y = np.zeros(max(n, 1), np.float32)
        check(lib().ptts_resample_ex(self.handle, fptr(x), x.size, int(sr_from), int(sr_to), code, fptr(y)))
        return y[:n]

    # -- slots
    def open(self, slot: int, voice: Voice, ids, params: GenerationParams):
        self.open_many([slot], [voice], [ids], [params])

    def open_many(self, slots, voices, ids_list, params_list):
        """Batched admission (ptts_slots_open_opts): row slots[i] <- (voices[i], ids_list[i], params_list[i])."""
        n = len(slots)
        sl = np.ascontiguousarray(np.asarray(slots, np.int32))
        arrs = [np.asarray(x, np.int32).reshape(-1) for x in ids_list]
        nid = np.ascontiguousarray(np.array([a.size for a in arrs], np.int32))
        cat = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0, np.int32))
        vh = (C.c_void_p * n)(*[v.handle for v in voices])
        ps = (GenParams * n)(*[p.to_c() for p in params_list])
        metered = any(getattr(p, "loudness", False) for p in params_list)  # one struct size per call: 72 bytes then
        rows = [p.slot_opts(self.lsd_decode_steps, metered) for p in params_list]  # (they keep the prefixes alive)
        opts = ((SlotOpts6 if metered else SlotOpts5) * n)(*rows)
        i32 = C.POINTER(C.c_int32)
        check(lib().ptts_slots_open_opts(self.handle, n, sl.ctypes.data_as(i32), vh, cat.ctypes.data_as(i32),
                                         nid.ctypes.data_as(i32), ps, C.cast(opts, C.c_void_p)))

    def close_slot(self, slot: int):
        check(lib().ptts_slot_close(self.handle, slot))

    def cancel_slots(self, slots):
        """Stop the utterances of these (distinct) slots without draining the pipeline
        (ptts_slots_cancel): returns at once, the other rows keep stepping, and no later fetch
        reports a frame of a cancelled utterance. The slots may be admitted again right away."""
        sl = np.ascontiguousarray(np.asarray(list(slots), np.int32).reshape(-1))
        check(lib().ptts_slots_cancel(self.handle, int(sl.size), sl.ctypes.data_as(C.POINTER(C.c_int32))))

    def set_latent(self, slot: int, latent: np.ndarray):
        v = np.ascontiguousarray(latent, np.float32).reshape(LDIM)
        check(lib().ptts_slot_set_latent(self.handle, slot, fptr(v)))

    def decode_latents(self, slot: int, latents: np.ndarray) -> dict:
        """MimiModel::decode_from_latent of n FlowLM latents [n, 32] on a reset slot (idle engine):
        pcm [n, 1920], quantized [n, 512], after_upsample / after_transformer [n, 16, 512]."""
        lat = np.ascontiguousarray(latents, np.float32).reshape(-1, LDIM)
        n = lat.shape[0]
        out = {"pcm": np.zeros((n, FRAME), np.float32), "quantized": np.zeros((n, 512), np.float32),
               "after_upsample": np.zeros((n, 16, 512), np.float32),
               "after_transformer": np.zeros((n, 16, 512), np.float32)}
        check(lib().ptts_decode_latents(self.handle, slot, fptr(lat), n, fptr(out["pcm"]), fptr(out["quantized"]),
                                        fptr(out["after_upsample"]), fptr(out["after_transformer"])))
        return out

    # -- the batched hot path
    def step(self, n_rows: int) -> StepResult:
        r = StepResult(np.zeros((n_rows, FRAME), np.float32), np.zeros(n_rows, np.uint8), np.zeros(n_rows, np.uint8),
                       np.zeros(n_rows, np.float32), np.zeros((n_rows, LDIM), np.float32))
        check(lib().ptts_step(self.handle, n_rows, fptr(r.pcm), u8ptr(r.valid), u8ptr(r.last), fptr(r.eos_logits),
                              fptr(r.latents)))
        r.valid = r.valid.astype(bool)
        r.last = r.last.astype(bool)
        return r

    def step_async(self, n_rows: int):
        check(lib().ptts_step_async(self.handle, n_rows))

    def flush_async(self, n_rows: int):
        """A pipelined call that starts no frame (ptts_flush_async): drains the frames already
        computed without running front parts whose frames would be discarded."""
        check(lib().ptts_flush_async(self.handle, n_rows))

    def sync(self):
        check(lib().ptts_sync(self.handle))

    def fetch(self, n_rows: int, calls_back: int = 0) -> StepResult:
        """Outputs of the latest call (calls_back = 0) or of the call before it (1: a driver that
        keeps one call in flight)."""
        r = StepResult(np.empty((n_rows, FRAME), np.float32), np.zeros(n_rows, np.uint8), np.zeros(n_rows, np.uint8),
                       np.zeros(n_rows, np.float32), np.zeros((n_rows, LDIM), np.float32))
        check(lib().ptts_fetch_prev(self.handle, calls_back, n_rows, fptr(r.pcm), u8ptr(r.valid), u8ptr(r.last),
                                    fptr(r.eos_logits), fptr(r.latents)))
        r.valid = r.valid.astype(bool)
        r.last = r.last.astype(bool)
        return r

    def fetch_wire(self, n_rows: int, calls_back: int = 0) -> list[bytes]:
        """The wire chunks of the frame fetch(n_rows, calls_back) returns (ptts_fetch_wire): one
        bytes object per row, empty for a row with no wire format or no frame."""
        if self._wire_buf is None:
            self._wire_buf = np.zeros((self.max_slots, self.wire_chunk_max), np.uint8)
            self._wire_n = np.zeros(self.max_slots, np.int32)
        check(lib().ptts_fetch_wire(self.handle, calls_back, n_rows, u8ptr(self._wire_buf), self.wire_chunk_max,
                                    self._wire_n.ctypes.data_as(C.POINTER(C.c_int))))
        return [self._wire_buf[b, : self._wire_n[b]].tobytes() for b in range(n_rows)]

    def fetch_loud(self, n_rows: int, calls_back: int = 0) -> list[np.ndarray]:
        """The loudness records of the frame fetch(n_rows, calls_back) returns (ptts_fetch_loud): one
        float64 array per row, the energies of the sub-blocks the row's frame completed (0 to 3),
        empty for a row that is not metered or has no frame. A row's arrays concatenated are
        audio.loudness_blocks of the signal its wire stage read; audio.loudness_integrated turns them
        into LUFS."""
        e = np.zeros((n_rows, 3), np.float64)
        nb = np.zeros(n_rows, np.int32)
        check(lib().ptts_fetch_loud(self.handle, calls_back, n_rows, e.ctypes.data_as(C.POINTER(C.c_double)),
                                    nb.ctypes.data_as(C.POINTER(C.c_int))))
        return [e[b, : nb[b]].copy() for b in range(n_rows)]

    def loudness_blocks(self, x: np.ndarray) -> np.ndarray:
        """Sub-block energies of a whole f32 signal at 24 kHz on the GPU (ptts_loud_blocks): the block
        function of the streaming loudness stage (audio.loudness_blocks is its host restatement)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        e = np.zeros(max(int(lib().ptts_loud_len(x.size)), 1), np.float64)
        check(lib().ptts_loud_blocks(self.handle, fptr(x), x.size, e.ctypes.data_as(C.POINTER(C.c_double))))
        return e[: x.size // 2400]

    def fetch_align(self, n_rows: int, calls_back: int = 0) -> list[np.ndarray]:
        """The alignment rows of the frame fetch(n_rows, calls_back) returns (ptts_fetch_align): one
        float32 array per row over the row's tokens, empty for a row with no valid frame or not in
        the align stage."""
        if self._align_buf is None:
            self._align_buf = np.zeros((self.max_slots, ALIGN_TOKENS), np.float32)
            self._align_n = np.zeros(self.max_slots, np.int32)
        check(lib().ptts_fetch_align(self.handle, calls_back, n_rows, fptr(self._align_buf), ALIGN_TOKENS,
                                     self._align_n.ctypes.data_as(C.POINTER(C.c_int))))
        return [self._align_buf[b, : self._align_n[b]].copy() for b in range(n_rows)]

    def encode_wire(self, pcm: np.ndarray, sample_rate: int = 24000, encoding="pcm_s16le") -> bytes:
        """Whole-signal f32 PCM at 24 kHz -> wire bytes on the GPU (ptts_wire_encode): the resampler
        of resample(), then the encoder of the streaming stage."""
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        enc = wire_encoding_code(encoding)
        n = int(lib().ptts_wire_len(x.size, int(sample_rate), enc))
        out = np.zeros(max(n, 1), np.uint8)
        check(lib().ptts_wire_encode(self.handle, fptr(x), x.size, int(sample_rate), enc, out.ctypes.data_as(U8P)))
        return out[:n].tobytes()

    def fetch_flac_index(self, n_rows: int, calls_back: int = 0) -> list[list[tuple[int, int]]]:
        """The frame index of the chunks fetch_wire(n_rows, calls_back) returns (ptts_fetch_flac_index;
        a FLAC-enabled engine): per row the (byte length, block size) of each frame of its chunk, empty
        for a row that is not FLAC or has no chunk. What audio.flac_rebase needs to renumber them."""
        idx = np.zeros((n_rows, 3, 2), np.int32)
        nf = np.zeros(n_rows, np.int32)
        check(lib().ptts_fetch_flac_index(self.handle, calls_back, n_rows, idx.ctypes.data_as(I32P), nf.ctypes.data_as(I32P)))
        return [[(int(a), int(b)) for a, b in idx[r, : nf[r]]] for r in range(n_rows)]

    def flac_encode(self, samples_i16: np.ndarray, sample_rate: int = 24000, first_sample: int = 0,
                    index: bool = False):
        """The FLAC stage's chunk encoder on up to 11,477 arbitrary 16-bit samples (ptts_flac_encode):
        the frames audio.flac_frames restates on the host, byte for byte. index=True
        (ptts_flac_encode_ex): (frames, [(byte length, block size) per frame])."""
        x = np.ascontiguousarray(np.asarray(samples_i16, np.int16).reshape(-1))
        out = np.zeros(max(int(lib().ptts_flac_bound(x.size)), 1), np.uint8)
        n = C.c_int(0)
        if not index:
            check(lib().ptts_flac_encode(self.handle, x.ctypes.data_as(C.POINTER(C.c_int16)), x.size, int(sample_rate),
                                         int(first_sample), out.ctypes.data_as(U8P), C.byref(n)))
            return out[: n.value].tobytes()
        idx, nf = np.zeros((3, 2), np.int32), C.c_int(0)
        check(lib().ptts_flac_encode_ex(self.handle, x.ctypes.data_as(C.POINTER(C.c_int16)), x.size, int(sample_rate),
                                        int(first_sample), out.ctypes.data_as(U8P), C.byref(n), idx.ctypes.data_as(I32P),
                                        C.byref(nf)))
        return out[: n.value].tobytes(), [(int(a), int(b)) for a, b in idx[: nf.value]]

    @staticmethod
    def tempo_len(n: int, speed) -> int:
        """Samples of an n-sample utterance at `speed` (ptts_tempo_len; host only)."""
        return int(lib().ptts_tempo_len(int(n), speed_permille(speed) or 1000))

    def tempo(self, pcm: np.ndarray, speed) -> np.ndarray:
        """Whole-signal f32 PCM at 24 kHz time-scaled by `speed` on the GPU (ptts_tempo): the rule of
        the streaming tempo stage (audio.tempo_wsola is its host restatement). Speed 1.0: a copy."""
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        sp = speed_permille(speed)
        if sp == 0:
            return x.copy()
        n = int(lib().ptts_tempo_len(x.size, sp))
        y = np.zeros(max(n, 1), np.float32)
        check(lib().ptts_tempo(self.handle, fptr(x), x.size, sp, fptr(y)))
        return y[:n]

    @staticmethod
    def pitch_len(n: int, step: int) -> int:
        """Samples of n inputs read at step / 2^20 inputs per output (ptts_pitch_len; host only)."""
        return int(lib().ptts_pitch_len(int(n), int(step)))

    def pitch_resample(self, x: np.ndarray, step: int) -> np.ndarray:
        """Whole-signal f32 read at step / 2^20 (Q20, 2^19 .. 2^21) inputs per output on the GPU
        (ptts_pitch_resample): the tap loop of the streaming pitch stage (audio.pitch_resample is its
        host restatement)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        n = self.pitch_len(x.size, step)
        y = np.zeros(max(n, 1), np.float32)
        check(lib().ptts_pitch_resample(self.handle, fptr(x), x.size, int(step), fptr(y)))
        return y[:n]

    def level(self, x: np.ndarray, gain_db: float, ceiling_db: float | None = None) -> np.ndarray:
        """Whole-signal f32 scaled by gain_db and peak-limited to ceiling_db (None: the engine's
        level_ceiling_db, -1.0 where the stage is off) on the GPU (ptts_level): the window function of
        the streaming level stage (audio.level_limit is its host restatement)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        if ceiling_db is None:
            ceil_cdb = self.level_ceiling_cdb if self.level_enabled else -100
        else:
            ceil_cdb = level_cdb(ceiling_db, -40.0, 0.0, "ceiling_db")
        y = np.zeros(max(x.size, 1), np.float32)
        check(lib().ptts_level(self.handle, fptr(x), x.size, level_cdb(gain_db), ceil_cdb, fptr(y)))
        return y[:x.size]

    def fetch_ready(self, calls_back: int = 0) -> bool:
        """fetch(calls_back=...) would not block (ptts_fetch_ready)."""
        r = C.c_int(0)
        check(lib().ptts_fetch_ready(self.handle, calls_back, C.byref(r)))
        return bool(r.value)

    def front_done(self, calls_back: int = 1, wait: bool = False) -> bool:
        """The FlowLM step of the call calls_back calls before the latest has run (ptts_front_done);
        wait=True blocks until it has."""
        r = C.c_int(0)
        check(lib().ptts_front_done(self.handle, calls_back, int(wait), C.byref(r)))
        return bool(r.value)

    def enable_preview(self, max_rows: int = 8):
        """First-frame previews (ptts_preview_enable, pipelined engines): the first frame of up to
        max_rows rows starting in one call is decoded right after their first FlowLM step, alone,
        so it does not wait frame_lag() calls; fetch_previews() returns them. 0 disables."""
        check(lib().ptts_preview_enable(self.handle, int(max_rows)))
        self._pv_slots = np.zeros(64, np.int32)
        self._pv_pcm = np.zeros((64, FRAME), np.float32)

    def fetch_previews(self, wait: bool = False) -> list[tuple[int, np.ndarray]]:
        """Completed first-frame previews, oldest first: (slot, pcm [1920]) pairs (fresh arrays).
        wait=False never blocks."""
        n = C.c_int(0)
        check(lib().ptts_preview_fetch(self.handle, int(wait), len(self._pv_slots),
                                       self._pv_slots.ctypes.data_as(C.POINTER(C.c_int)), fptr(self._pv_pcm),
                                       C.byref(n)))
        return [(int(self._pv_slots[i]), self._pv_pcm[i].copy()) for i in range(n.value)]

    def generate(self, slot: int, voice: Voice, ids, params: GenerationParams) -> np.ndarray:
        if self._row_lsd(params) != self.max_lsd_steps:
            # ptts_generate admits at the engine's cap: its loop here, over an admission at the row's count
            self.open(slot, voice, ids, params)
            lag, delay = self.frame_lag()
            frames = []
            for it in range(params.max_frames + lag + delay):
                r = self.step(slot + 1)
                if not r.valid[slot]:
                    if it < lag + delay:
                        continue
                    break
                frames.append(r.pcm[slot].copy())
                if r.last[slot]:
                    break
            return np.concatenate(frames) if frames else np.zeros(0, np.float32)
        a = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        cap = params.max_frames * FRAME
        out = np.zeros(cap, np.float32)
        n = C.c_int(0)
        cp = params.to_c()
        check(lib().ptts_generate(self.handle, slot, voice.handle, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size,
                                  C.byref(cp), fptr(out), cap, C.byref(n)))
        return out[: n.value]

    # -- measurement
    def plan(self, n_rows: int) -> list[tuple[str, float, float]]:
        """The step plan: (op name, algorithmic flops, algorithmic bytes) per launch."""
        buf = C.create_string_buffer(1 << 17)
        check(lib().ptts_plan_ops(self.handle, n_rows, buf, len(buf)))
        out = []
        for line in buf.value.decode().split("\n"):
            if line:
                name, fl, by = line.split("\t")
                out.append((name, float(fl), float(by)))
        return out

    def plan_ops(self, n_rows: int) -> list[str]:
        return [n for n, _, _ in self.plan(n_rows)]

    def time_kernel(self, n_rows: int, name: str, reps: int = 50) -> float:
        us = C.c_double(0)
        check(lib().ptts_time_kernel(self.handle, n_rows, name.encode(), reps, C.byref(us)))
        return us.value
