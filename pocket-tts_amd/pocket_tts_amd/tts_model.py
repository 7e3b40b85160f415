"""Host-side mirror of the reference's `TTSModel` API (crates/pocket-tts/src/tts_model.rs),
running the generation hot path through the HIP engine.

Reference surface kept:
  * `TTSModel.load / load_with_params`, public fields `temp`, `lsd_decode_steps`,
    `eos_threshold`, `noise_clamp`, `sample_rate`, `voice_prompt_chunk_frames` (:22-49, :417), all
    live: each segment is generated with the values the fields hold when it starts
    (`lsd_decode_steps` up to the engine's cap, `max_lsd_decode_steps` at load);
  * voices: `get_voice_state` (:446-463), `get_voice_state_from_bytes` (:428-444),
    `get_voice_state_from_tensor` (:504-577), `get_voice_state_from_prompt_file / _bytes /
    _tensor` (:465-501). WAV decode on the host (audio.py), resampling and the Mimi encoder on
    the GPU;
  * generation: `generate` (:687-703), `generate_stream` (:894-913: sentence chunks of at most
    50 tokens, one segment each from a fresh copy of the voice state), `generate_stream_long`
    and `generate_with_pauses` (:856-883, 1074-1131: pause markers become silence), one
    [1, 1, 1920] frame per item; `split_into_best_sentences` (:601-684),
    `estimate_generation_steps` (:1187-1190);
  * `generate_parallel` / `generate_stream_parallel` (:705-854, commented out in the reference):
    the same segments as rows of one batch, on an engine loaded with `max_slots` > 1.
Not in the reference: `generate(.., timestamps=True)` and `generate_parallel(.., timestamps=True)`
return `(audio, words)`, the words with their start and end in seconds of that audio (align.py;
DESIGN.md section 26), on a model loaded with `align=True`.
Text goes through the text front end (text.py: tokenizer, prompt preparation); token-id input
is accepted too (one segment, no splitting).
"""

from __future__ import annotations

import math
import weakref
from dataclasses import dataclass
from typing import Callable, Iterator, Sequence

import numpy as np

from ._lib import FRAME, QUANT_ALL, QUANT_FLOW_LM, QUANT_NONE, SAMPLE_RATE
from .audio import (FlacJoiner, flac_stream_header, loudness_gain_cdb, loudness_integrated, read_wav,
                    read_wav_from_bytes, wire_bytes)
from . import align as _align
from .engine import Engine, GenerationParams, OutputOptions, Voice
from .text import (CALIBRATION_SEED, CALIBRATION_TEXT, estimate_frames_after_eos, load_tokenizer, long_form_segments, long_text_segments, max_gen_len,
                   prepare_text_prompt, segment_request, silence_samples, split_into_best_sentences)

DEFAULT_VARIANT = "b6369a24"

__all__ = ["TTSModel", "Continuation", "prepare_text_prompt", "estimate_frames_after_eos", "max_gen_len",
           "DEFAULT_VARIANT"]


@dataclass
class Continuation:
    """What the next link of a continuity chain needs of the one before it (generate_continued;
    DESIGN.md section 20): the segment's own token ids, the latents of every frame it delivered
    (its EOS tail included) and the engine slot whose codec state it ended on."""

    ids: np.ndarray
    latents: np.ndarray
    slot: int = 0


def _mono(audio: np.ndarray) -> np.ndarray:
    """[channels, n] -> [n]. The reference's Mimi encoder has one input channel, so a multi-channel
    prompt is an error there too (get_voice_state_from_tensor on [1, C, T])."""
    if audio.shape[0] != 1:
        raise ValueError(f"voice prompt must be mono, got {audio.shape[0]} channels")
    return audio[0]


class TTSModel:
    def __init__(self, engine: Engine, temp: float, lsd_decode_steps: int, eos_threshold: float,
                 noise_clamp: float | None, tokenizer: Callable[[str], Sequence[int]] | None = None):
        self.engine = engine
        self.temp = temp
        self.lsd_decode_steps = lsd_decode_steps
        self.eos_threshold = eos_threshold
        self.noise_clamp = noise_clamp
        self.sample_rate = SAMPLE_RATE
        self.tokenizer = tokenizer
        self.voice_prompt_chunk_frames: int | None = None  # tts_model.rs:417 (None = adaptive rule)
        # voice-prompt resampler for rates other than 24 kHz: "poly" (resample_poly, the rule of the
        # reference's ref.wav fixture pair) or "rubato" (the Rust driver's FastFixedIn / Septic,
        # audio.rs:197-255; restated, parity unpinned)
        self.voice_resampler: str = "poly"
        self._seed = 0
        # Voice -> LUFS or None (voice_loudness); weak, so a value dies with its Voice object
        self._voice_loudness: weakref.WeakKeyDictionary = weakref.WeakKeyDictionary()

    @classmethod
    def load(cls, variant: str = DEFAULT_VARIANT, **kw) -> "TTSModel":
        return cls.load_with_params(variant, **kw)

    @classmethod
    def load_with_params(cls, variant: str = DEFAULT_VARIANT, temp: float = 0.7, lsd_decode_steps: int = 1,
                         eos_threshold: float = -4.0, noise_clamp: float | None = None, *,
                         weights_path: str | None = None, tokenizer_path: str | None = None, seed: int = 0x5EED,
                         device: int = 0, max_ctx: int = 1024, tokenizer=None,
                         weight_quant: int = QUANT_NONE, max_lsd_decode_steps: int | None = None,
                         wire: bool = False, max_slots: int = 1, pipeline: bool = False,
                         back_frames: int = 1, tempo: bool = False, flac: bool = False,
                         pitch: bool = False, level: bool = False, level_ceiling_db: float = -1.0,
                         align: bool = False, align_layer: int = 0, align_heads: int = 0xFFFF,
                         loud: bool = False) -> "TTSModel":
        """max_slots: the engine's row count (generate_parallel runs a text's segments on them; the
        other methods use row 0). pipeline / back_frames: overlapped stepping (Engine).
        max_lsd_decode_steps: the largest value the `lsd_decode_steps` field may later be set to
        (the engine's cap; None: lsd_decode_steps itself, the field can then only be lowered).
        weights_path: local safetensors with the TTSModel state-dict names (synthetic weights
        from `seed` when None); tokenizer_path: tokenizer.model (SentencePiece) or tokenizer.json.
        wire: a wire-enabled engine, for generate(.., sample_rate=, encoding=); tempo (with wire):
        its tempo stage too, for generate(.., speed=); pitch (with tempo): its pitch stage, for
        generate(.., pitch=); flac (with wire): its FLAC stage, for
        generate(.., encoding="flac"); level (with wire): its level stage at level_ceiling_db, for
        generate(.., volume_db=, limit=). align: its align stage on FlowLM layer align_layer over the
        heads of the mask align_heads, for generate(.., timestamps=True). loud (with wire): its
        loudness stage, for generate(.., measure_loudness=True) and, with level, loudness_lufs=."""
        if variant != DEFAULT_VARIANT:
            raise ValueError(f"unsupported variant {variant!r} (only {DEFAULT_VARIANT})")
        if tokenizer is None and tokenizer_path:
            tokenizer = load_tokenizer(tokenizer_path)
        eng = Engine(device=device, max_slots=int(max_slots), max_ctx=max_ctx, pipeline=pipeline,
                     back_frames=back_frames, lsd_decode_steps=lsd_decode_steps, seed=seed,
                     weights_path=weights_path, weight_quant=weight_quant, max_lsd_steps=max_lsd_decode_steps,
                     wire=wire, tempo=tempo, flac=flac, pitch=pitch,
                     **(dict(level=True, level_ceiling_db=level_ceiling_db) if level else {}),
                     **(dict(align=True, align_layer=align_layer, align_heads=align_heads) if align else {}),
                     **(dict(loud=True) if loud else {}))
        return cls(eng, temp, lsd_decode_steps, eos_threshold, noise_clamp, tokenizer)

    # ---- quantized loading (tts_model.rs:108-181, feature "quantized"). The reference's version
    # is a placeholder that returns the f32 model (is_quantized() == false); here the weights get
    # quantize_weights() with QuantizeConfig::default() (quantize.rs) and the FlowLM step GEMMs
    # stream the int8 codes. scope: QUANT_FLOW_LM (default) or QUANT_ALL.
    @classmethod
    def load_quantized(cls, variant: str = DEFAULT_VARIANT, **kw) -> "TTSModel":
        return cls.load_quantized_with_params(variant, **kw)

    @classmethod
    def load_quantized_with_params(cls, variant: str = DEFAULT_VARIANT, temp: float = 0.7,
                                   lsd_decode_steps: int = 1, eos_threshold: float = -4.0,
                                   noise_clamp: float | None = None, *, scope: int = QUANT_FLOW_LM,
                                   **kw) -> "TTSModel":
        if scope not in (QUANT_FLOW_LM, QUANT_ALL):
            raise ValueError("scope must be QUANT_FLOW_LM or QUANT_ALL")
        return cls.load_with_params(variant, temp, lsd_decode_steps, eos_threshold, noise_clamp,
                                    weight_quant=scope, **kw)

    def is_quantized(self) -> bool:
        return self.engine.weight_quant != QUANT_NONE

    # ---- voice states
    def get_voice_state_from_prompt_tensor(self, prompt: np.ndarray) -> Voice:
        return self.engine.voice_from_prompt(np.asarray(prompt, np.float32).reshape(-1, 1024))

    def get_voice_state_from_tensor(self, audio: np.ndarray, sample_rate: int = SAMPLE_RATE) -> Voice:
        """tts_model.rs:504-577 (24 kHz mono PCM); other rates are resampled on the GPU first."""
        return self.engine.voice_from_audio(np.asarray(audio, np.float32).reshape(-1), sample_rate,
                                            self.voice_prompt_chunk_frames or 0, self.voice_resampler)

    def get_voice_state_from_bytes(self, data: bytes) -> Voice:
        """tts_model.rs:428-444: WAV bytes -> (GPU) resample -> encode -> prompt prefill."""
        audio, sr = read_wav_from_bytes(data)
        return self.get_voice_state_from_tensor(_mono(audio), sr)

    def get_voice_state(self, path: str) -> Voice:
        """tts_model.rs:446-463."""
        audio, sr = read_wav(path)
        return self.get_voice_state_from_tensor(_mono(audio), sr)

    def get_voice_state_from_prompt_file(self, path: str) -> Voice:
        """tts_model.rs:465-477: a safetensors file holding `audio_prompt` [1, F, 1024]."""
        from safetensors.numpy import load_file

        t = load_file(str(path))
        if "audio_prompt" not in t:
            raise KeyError("'audio_prompt' not found in safetensors file")
        return self.get_voice_state_from_prompt_tensor(t["audio_prompt"])

    def get_voice_state_from_prompt_bytes(self, data: bytes) -> Voice:
        """tts_model.rs:479-487."""
        from safetensors.numpy import load

        t = load(data)
        if "audio_prompt" not in t:
            raise KeyError("'audio_prompt' not found in safetensors bytes")
        return self.get_voice_state_from_prompt_tensor(t["audio_prompt"])

    # ---- text
    def _tok(self):
        if self.tokenizer is None:
            raise ValueError("text input needs a tokenizer (TTSModel.load(..., tokenizer_path=...) or "
                             "tokenizer=callable); or pass token ids")
        return self.tokenizer

    def count_tokens(self, text: str) -> int:
        tok = self._tok()
        return tok.count_tokens(text) if hasattr(tok, "count_tokens") else len(tok(text))

    def split_into_best_sentences(self, text: str) -> list[str]:
        return split_into_best_sentences(text, self.count_tokens)

    def estimate_generation_steps(self, text: str) -> int:
        return max_gen_len(prepare_text_prompt(text))

    # ---- generation
    def _params(self, max_frames: int, frames_after_eos: int, seed: int | None = None) -> GenerationParams:
        """seed: the row's own seed (the calibration row); None: the next of the model's counter."""
        if seed is None:
            self._seed += 1
            seed = self._seed
        return GenerationParams(temp=self.temp, eos_threshold=self.eos_threshold, noise_clamp=self.noise_clamp,
                                frames_after_eos=frames_after_eos, max_frames=max_frames, seed=seed)

    def _check_lsd(self):
        cap = self.engine.max_lsd_steps
        if not 1 <= int(self.lsd_decode_steps) <= cap:
            raise ValueError(f"lsd_decode_steps {self.lsd_decode_steps} outside [1, {cap}], the engine's cap "
                             "(max_lsd_decode_steps at load)")

    def _segment(self, ids: np.ndarray, voice_state: Voice, max_frames: int, frames_after_eos: int,
                 out: OutputOptions = OutputOptions(), previous: Continuation | None = None,
                 latents: list | None = None, align: list | None = None,
                 joiner: FlacJoiner | None = None, loud: list | None = None,
                 seed: int | None = None) -> Iterator[np.ndarray]:
        """generate_stream_segment (tts_model.rs:935-1071) on engine row 0. For a wire row (out.wire:
        a format on a wire-enabled engine, a speed on a tempo-enabled one, a pitch, a gain or limit
        likewise) the items are the row's wire chunks, bytes converted on the GPU (Engine.fetch_wire),
        instead of f32 frames.
        previous: the segment continues that one (section 20): admitted behind its ids and, as a
        teacher-forced prefix, its latents, on the codec state it left (only the new frames are
        yielded); where that exceeds the engine's max_ctx, as a plain segment. latents: a list that
        receives the latent of every frame yielded. align: a list that receives the alignment row of
        every frame yielded (an align-enabled engine; the row is admitted with align). joiner (a FLAC
        row): the chunks are renumbered to the segment's place in the joiner's stream (section 21.5),
        and the segment is closed there when it ends. loud: a list that receives the sub-block
        energies of every frame yielded (a loudness-enabled engine; the row is admitted metered).
        seed: the row's seed in place of the model's counter, which then stays as it is."""
        self._check_lsd()
        params = out.apply(self._params(max_frames, frames_after_eos, seed))
        params.lsd_steps = int(self.lsd_decode_steps)
        params.align = align is not None
        params.loudness = loud is not None
        if previous is not None and (voice_state.n_frames + previous.ids.size + ids.size + len(previous.latents)
                                     + max_frames <= self.engine.max_ctx):
            ids = np.concatenate([np.asarray(previous.ids, np.int32), ids])
            params.prefix_latents, params.keep_codec = np.asarray(previous.latents, np.float32), True
        wire = out.wire is not None
        self.engine.open(0, voice_state, ids, params)
        lag, delay = self.engine.frame_lag()  # overlapped stepping: frames arrive lag (+ delay) calls late
        lead = lag + delay
        try:
            while True:
                r = self.engine.step(1)
                if not r.valid[0]:
                    if lead > 0:
                        lead -= 1
                        continue
                    return
                lead = 0
                if latents is not None:
                    latents.append(np.array(r.latents[0], np.float32))
                if align is not None:
                    align.append(self.engine.fetch_align(1)[0])
                if loud is not None:
                    loud.append(self.engine.fetch_loud(1)[0])
                if joiner is not None:
                    yield joiner.chunk(self.engine.fetch_wire(1)[0], self.engine.fetch_flac_index(1)[0])
                else:
                    yield self.engine.fetch_wire(1)[0] if wire else r.pcm[0].reshape(1, 1, FRAME).copy()
                if r.last[0]:
                    return
        finally:
            if joiner is not None:
                joiner.end_segment()

    def generate_stream(self, text_or_ids, voice_state: Voice, max_frames: int | None = None,
                        words: int | None = None, sample_rate: int | None = None, encoding=None,
                        speed: float | None = None, pitch: float | None = None, volume_db: float | None = None,
                        limit: bool = False) -> Iterator[np.ndarray]:
        """tts_model.rs:894-913. Text: one segment per sentence chunk; max_gen_len and the EOS tail
        from each chunk (:968-969). Token ids (an extension for callers with their own tokenizer):
        one segment; ids carry no word count, so the caller passes `words` (the reference's rules
        then apply: max_gen_len = (words + 2) * 13, tail 5 frames up to 4 words else 3) or an
        explicit max_frames (tail 3).
        sample_rate (8000, 16000, 24000, 44100, 48000) and / or encoding ("pcm_s16le", "ulaw",
        "alaw"): the items are bytes in that wire format, one chunk per frame (every segment is
        resampled on its own: its chunks are the whole-signal resample of the segment).
        speed (0.5 .. 2.0; a tempo-enabled engine): the segments' audio is time-scaled on the GPU
        ahead of that conversion, pitch kept; the items are wire bytes then
        too, 24 kHz 16-bit unless a format is given. None or 1.0 changes nothing.
        pitch (-12 .. 12 semitones; a pitch-enabled engine): the segments' audio is shifted in pitch
        on the GPU at the duration `speed` asks for, a resampling shift that moves the formants too
        (DESIGN.md section 23); wire bytes as for speed. None or 0 changes nothing.
        volume_db (-24 .. 24 dB) and limit (a level-enabled engine): the segments' audio is scaled and
        run through the look-ahead peak limiter on the GPU, behind speed and pitch (DESIGN.md section
        24); wire bytes as for speed. None / 0 with limit False changes nothing.
        encoding "flac" (a FLAC-enabled engine): the items are the FLAC frames of each chunk (DESIGN.md
        section 21), to be sent behind audio.flac_stream_header. A row numbers its samples from 0; the
        frames of every segment after the first are renumbered on the host to follow the one before
        (audio.FlacJoiner, section 21.5), so the items are one stream."""
        yield from self._stream(text_or_ids, voice_state, max_frames, words,
                                OutputOptions.of(sample_rate, encoding, speed, pitch, volume_db, limit))

    @staticmethod
    def _joiner(out: OutputOptions) -> FlacJoiner | None:
        """The joiner of a FLAC response (None: another format)."""
        return FlacJoiner(out.wire[0]) if out.wire and out.wire[1] == "flac" else None

    def _stream(self, text_or_ids, voice_state, max_frames, words, out: OutputOptions,
                joiner: FlacJoiner | None = None, loud: list | None = None) -> Iterator[np.ndarray]:
        """loud: a list that receives, per segment (a row of its own), the list of its frames' energies."""
        joiner = joiner or self._joiner(out)

        def row():
            if loud is None:
                return None
            loud.append([])
            return loud[-1]

        if not isinstance(text_or_ids, str):
            ids = np.asarray(text_or_ids, np.int32).reshape(-1)
            if words is None and max_frames is None:
                raise ValueError("token ids carry no word count: pass words= or max_frames=")
            fae = 3 if words is None else (5 if words <= 4 else 3)
            yield from self._segment(ids, voice_state, max_frames or (words + 2) * 13, fae, out, joiner=joiner,
                                     loud=row())
            return
        tok = self._tok()
        for chunk in self.split_into_best_sentences(text_or_ids):
            prepared = prepare_text_prompt(chunk)
            ids = np.asarray(tok(prepared), np.int32)
            yield from self._segment(ids, voice_state, max_frames or max_gen_len(prepared),
                                     estimate_frames_after_eos(chunk), out, joiner=joiner, loud=row())

    def generate(self, text_or_ids, voice_state: Voice, max_frames: int | None = None,
                 words: int | None = None, sample_rate: int | None = None, encoding=None,
                 speed: float | None = None, pitch: float | None = None, volume_db: float | None = None,
                 limit: bool = False, timestamps: bool = False, measure_loudness: bool = False,
                 loudness_lufs: float | None = None):
        """tts_model.rs:687-703: all frames concatenated, [1, N*1920]; with sample_rate / encoding /
        speed / pitch / volume_db / limit, the wire bytes of generate_stream concatenated. encoding "flac": a complete .flac file,
        the stream header with the true sample count and then the frames (of every segment, joined).
        timestamps=True (text input, a model loaded with align=True and a tokenizer that names its
        pieces): returns (audio, words), words = [{"word", "start", "end"}] in seconds of that audio
        (align.py: each sentence chunk's words offset by the audio delivered before it).
        measure_loudness=True (a loudness-enabled engine): returns (audio, lufs),
        the integrated loudness of what the wire stage read (the 24 kHz signal behind speed, pitch
        and level), gated once over all segments; None where it is unmeasurable.
        loudness_lufs (-40 .. -5; a level- and loudness-enabled engine): the audio gets the constant
        gain target - voice_loudness(voice_state), within +-24 dB, through the level stage (so it is
        wire bytes); it excludes volume_db. ValueError for a voice whose calibration is unmeasurable."""
        if loudness_lufs is not None:
            if volume_db is not None:
                raise ValueError("loudness_lufs and volume_db exclude each other")
            t = float(loudness_lufs)
            if not (math.isfinite(t) and -40.0 <= t <= -5.0):
                raise ValueError(f"loudness_lufs must be in [-40, -5], got {loudness_lufs!r}")
            cal = self.voice_loudness(voice_state)
            if cal is None:
                raise ValueError("the voice's loudness is unmeasurable: no loudness target for it")
            volume_db, limit = loudness_gain_cdb(t, cal) / 100.0, True
        out = OutputOptions.of(sample_rate, encoding, speed, pitch, volume_db, limit)
        if timestamps:
            if measure_loudness:
                raise ValueError("measure_loudness with timestamps is not available here")
            return self._generate_timed(text_or_ids, voice_state, max_frames, out)
        joiner = self._joiner(out)
        loud = [] if measure_loudness else None
        frames = list(self._stream(text_or_ids, voice_state, max_frames, words, out, joiner, loud))
        if not frames:
            raise RuntimeError("No audio generated")
        if joiner is not None:
            audio = flac_stream_header(joiner.rate, joiner.total) + b"".join(frames)
        else:
            audio = b"".join(frames) if out.wire else np.concatenate(frames, axis=2)[0]
        if not measure_loudness:
            return audio
        rows = [np.concatenate(r) if r else np.zeros(0, np.float64) for r in loud]
        return audio, loudness_integrated(rows)

    def voice_loudness(self, voice_state: Voice) -> float | None:
        """The voice's integrated loudness in LUFS, measured on the GPU: the calibration the server
        runs. One row says text.CALIBRATION_TEXT at the model's parameters with
        the seed text.CALIBRATION_SEED, no gain, metered. The model's seed counter is not touched, so
        the value does not depend on what was generated before and later calls get the seeds they
        would have got without it. None: unmeasurable. Kept with the Voice object."""
        if voice_state not in self._voice_loudness:
            ids, mgl, fae = segment_request(CALIBRATION_TEXT, self._tok())
            loud: list = []
            for _ in self._segment(np.asarray(ids, np.int32), voice_state, mgl, fae, loud=loud, seed=CALIBRATION_SEED):
                pass
            energy = np.concatenate(loud) if loud else np.zeros(0, np.float64)
            self._voice_loudness[voice_state] = loudness_integrated(energy)
        return self._voice_loudness[voice_state]

    def _units(self, chunk, encoding) -> int:
        """Samples of one delivered item at the rate it is delivered at (f32 frames: 24 kHz)."""
        if not isinstance(chunk, (bytes, bytearray)):
            return int(np.asarray(chunk).shape[-1])
        return len(chunk) // (1 if encoding in ("ulaw", "alaw") else 2)

    def _words_of(self, ids, rows, n_frames, max_frames, fae, speed, seconds) -> list[dict]:
        """The words of one segment over its own audio of `seconds`: the EOS frame is the frame the
        tail of frames_after_eos frames began at, where the row ended before max_frames."""
        tok = self._tok()
        if not hasattr(tok, "pieces"):
            raise ValueError("timestamps need a tokenizer that names its pieces (text.Tokenizer)")
        A = np.zeros((n_frames, len(ids)), np.float64)
        for t, r in enumerate(rows[:n_frames]):
            A[t, :len(r)] = r[:len(ids)]
        eos = max(n_frames - fae, 0) if n_frames < max_frames else None
        return _align.timestamps(tok, ids, A, speed or 1.0, eos, seconds)

    def _generate_timed(self, text, voice_state, max_frames, out: OutputOptions):
        if not isinstance(text, str):
            raise ValueError("timestamps: token ids carry no words, pass text")
        if not self.engine.align_enabled:
            raise ValueError("timestamps need a model loaded with align=True")
        rate, enc = out.wire or (SAMPLE_RATE, None)
        if enc == "flac":
            raise ValueError("timestamps: not with flac (ask for pcm_s16le and encode the result)")
        tok = self._tok()
        chunks, words, at = [], [], 0.0
        for chunk in self.split_into_best_sentences(text):
            prepared = prepare_text_prompt(chunk)
            ids = np.asarray(tok(prepared), np.int32)
            mf, fae, rows = max_frames or max_gen_len(prepared), estimate_frames_after_eos(chunk), []
            frames = list(self._segment(ids, voice_state, mf, fae, out, align=rows))
            seconds = sum(self._units(f, enc) for f in frames) / rate
            for w in self._words_of(ids, rows, len(frames), mf, fae, out.speed, seconds):
                words.append({"word": w["word"], "start": round(w["start"] + at, 6), "end": round(w["end"] + at, 6)})
            at += seconds
            chunks += frames
        if not chunks:
            raise RuntimeError("No audio generated")
        return (b"".join(chunks) if out.wire else np.concatenate(chunks, axis=2)[0]), words

    def generate_stream_long(self, text: str, voice_state: Voice, continuity: bool = False,
                             sample_rate: int | None = None, encoding=None,
                             joiner: FlacJoiner | None = None) -> Iterator[np.ndarray]:
        """tts_model.rs:1074-1131: text segments between pause markers, silence for each pause.
        continuity (what tts_model.py:397-400 of the reference names and leaves
        out): the sentence chunks of one text piece run one after another on one slot, chunk k+1
        admitted with ids = ids(chunk k) ++ ids(chunk k+1), every delivered latent of chunk k as a
        teacher-forced prefix and keep_codec, so neither the prosody nor the codec restarts at the
        join; only the new frames are yielded. A pause starts a new chain.
        sample_rate / encoding: wire bytes as generate_stream yields them, each pause as the encoded
        silence of silence_samples(ms, sample_rate) samples. encoding "flac": one stream, to be sent
        behind audio.flac_stream_header; the pauses are CONSTANT frames (section 21.5). joiner: the
        FlacJoiner to use (generate_with_pauses reads its total)."""
        out = OutputOptions.of(sample_rate, encoding)
        joiner = joiner or self._joiner(out)
        for kind, val in long_text_segments(text):
            if kind != "text":
                if joiner is not None:
                    yield joiner.pause(silence_samples(val, joiner.rate))
                elif out.wire:
                    yield wire_bytes(np.zeros(silence_samples(val, out.wire[0]), np.float32), out.wire[1])
                else:
                    yield np.zeros((1, 1, silence_samples(val, self.sample_rate)), np.float32)
            elif not continuity:
                yield from self._stream(val, voice_state, None, None, out, joiner)
            else:
                prev = None
                for chunk in self.split_into_best_sentences(val):
                    link = self._link(chunk, voice_state, prev, out, joiner)
                    yield from link
                    prev = link.continuation

    def _link(self, chunk: str, voice_state: Voice, previous: Continuation | None,
              out: OutputOptions = OutputOptions(), joiner: FlacJoiner | None = None):
        """One sentence chunk as a link of a continuity chain: an iterator over its frames whose
        `continuation` is complete once it is exhausted."""
        prepared = prepare_text_prompt(chunk)
        ids = np.asarray(self._tok()(prepared), np.int32)
        lat: list = []
        frames = self._segment(ids, voice_state, max_gen_len(prepared), estimate_frames_after_eos(chunk), out,
                               previous=previous, latents=lat, joiner=joiner)

        class Link:
            continuation = None

            def __iter__(link):
                yield from frames
                link.continuation = Continuation(ids, np.array(lat, np.float32).reshape(-1, 32), 0)

        return Link()

    def generate_continued(self, text: str, voice_state: Voice, previous: Continuation | None = None,
                           sample_rate: int | None = None, encoding=None,
                           joiner: FlacJoiner | None = None) -> tuple[np.ndarray, Continuation]:
        """One link of a continuity chain (section 20): `text` as ONE segment (no sentence split),
        continuing `previous` (the Continuation an earlier call returned; None: a plain segment).
        Returns the new audio [1, N*1920] and the Continuation to hand to the next call. The chain
        lives on engine row 0: nothing else may be generated on this model between two links that
        are to join seamlessly. sample_rate / encoding: the new audio as wire bytes. encoding "flac":
        the link's frames alone (no stream header), numbered on from joiner.total where the caller
        hands the same audio.FlacJoiner to every link of the chain, from 0 without one."""
        out = OutputOptions.of(sample_rate, encoding)
        link = self._link(text, voice_state, previous, out, joiner or self._joiner(out))
        frames = list(link)
        if not frames:
            raise RuntimeError("No audio generated")
        return (b"".join(frames) if out.wire else np.concatenate(frames, axis=2)[0]), link.continuation

    def generate_with_pauses(self, text: str, voice_state: Voice, continuity: bool = False,
                             sample_rate: int | None = None, encoding=None):
        """tts_model.rs:856-883. sample_rate / encoding: the wire bytes of generate_stream_long joined;
        encoding "flac": a complete .flac file with the true sample count."""
        out = OutputOptions.of(sample_rate, encoding)
        joiner = self._joiner(out)
        chunks = list(self.generate_stream_long(text, voice_state, continuity, sample_rate, encoding, joiner))
        if not chunks:
            raise RuntimeError("No audio generated")
        if joiner is not None:
            return flac_stream_header(joiner.rate, joiner.total) + b"".join(chunks)
        return b"".join(chunks) if out.wire else np.concatenate(chunks, axis=2)[0]

    # ---- the same segments on parallel rows
    def generate_stream_parallel(self, text: str, voice_state: Voice, pauses: bool = False, rows: int | None = None,
                                 sample_rate: int | None = None, encoding=None,
                                 speed: float | None = None, pitch: float | None = None,
                                 timed: list | None = None) -> Iterator:
        """The items of generate_stream (pauses=False) or generate_stream_long (pauses=True), in text
        order, with the text segments generated as rows of one batch: up to `rows` (default: the
        engine's max_slots) are admitted at once (Engine.open_many: one shared text prefill, the
        voice prefix shared) and rows are refilled as segments end. The segments are independent
        utterances (each starts from the voice prefix with a fresh Mimi state, tts_model.rs:935-1004)
        and the noise of an utterance depends on its seed alone, not on its row, so segment i is the
        segment the sequential methods produce: it gets their seed (`_seed` advanced once per text
        segment, in text order) and the field values read when this call starts.
        sample_rate / encoding: wire bytes as generate_stream yields them, and each pause as the
        encoded silence of silence_samples(ms, sample_rate) samples. speed: every text segment's row
        carries it (generate_stream), and the pitch likewise; pauses keep their stated duration. Closing the generator early
        cancels the rows it still holds (Engine.cancel_slots). encoding "flac": the rows' chunks travel
        with their frame index and are renumbered as they are delivered in text order, the pauses
        are CONSTANT frames: one stream behind audio.flac_stream_header (section 21.5).
        timed: a list that receives one record per item, in text order (generate_parallel's
        timestamps): ("pause", samples) or ("text", ids, params, frames_after_eos, meta), meta the
        segment's alignment rows, frame count and delivered samples, complete once it is delivered;
        the text rows are then admitted with align."""
        return self._stream_parallel(text, voice_state, pauses, rows, OutputOptions.of(sample_rate, encoding, speed, pitch),
                                     timed)

    def _stream_parallel(self, text, voice_state, pauses, rows, out: OutputOptions, timed,
                         joiner: FlacJoiner | None = None) -> Iterator:
        self._check_lsd()
        wire = out.wire
        joiner = joiner or self._joiner(out)
        if joiner is not None and timed is not None:
            raise ValueError("timestamps: not with flac (ask for pcm_s16le and encode the result)")
        tok = self._tok()
        eng = self.engine
        n_rows = max(1, min(int(rows or eng.max_slots), eng.max_slots))
        items = []  # per segment: ("pause", item) | ["text", ids, params, frames, done]
        for kind, val in long_form_segments(text, self.count_tokens, pauses):
            if kind == "text":
                ids, mgl, fae = segment_request(val, tok)
                params = out.apply(self._params(mgl, fae))
                params.lsd_steps = int(self.lsd_decode_steps)
                params.align = timed is not None
                meta = {"rows": [], "frames": 0, "units": 0, "encoding": wire and wire[1]}
                items.append(["text", np.asarray(ids, np.int32), params, [], False, meta if timed is not None else None])
                if timed is not None:
                    timed.append(("text", items[-1][1], params, fae, meta))
            elif joiner is not None:
                items.append(("pause", silence_samples(val, wire[0])))  # encoded where it is delivered: at its place
            elif wire:
                n = silence_samples(val, wire[0])
                items.append(("pause", wire_bytes(np.zeros(n, np.float32), wire[1])))
                if timed is not None:
                    timed.append(("pause", n))
            else:
                items.append(("pause", np.zeros((1, 1, silence_samples(val, self.sample_rate)), np.float32)))
                if timed is not None:
                    timed.append(("pause", silence_samples(val, self.sample_rate)))
        return self._run_parallel(items, voice_state, n_rows, wire is not None, joiner)

    def _run_parallel(self, items, voice_state: Voice, n_rows: int, wire: bool,
                      joiner: FlacJoiner | None = None) -> Iterator:
        """joiner: the rows are FLAC; a segment's items are held as (chunk, index) and pass through the
        joiner, pauses too, as they are delivered."""
        eng = self.engine
        todo = [it for it in items if it[0] == "text"]  # not yet admitted, text order
        active: dict[int, list] = {}  # slot -> its segment
        lead: dict[int, int] = {}     # slot -> calls its first frame may still be late (frame_lag)
        head = 0
        try:
            while True:
                while head < len(items):  # deliver, strictly in text order
                    it = items[head]
                    if it[0] == "pause":
                        yield joiner.pause(it[1]) if joiner is not None else it[1]
                    else:
                        while it[3]:
                            yield joiner.chunk(*it[3].pop(0)) if joiner is not None else it[3].pop(0)
                        if not it[4]:
                            break
                        if joiner is not None:
                            joiner.end_segment()
                    head += 1
                if head == len(items):
                    return
                free = [s for s in range(n_rows) if s not in active]
                batch = [(s, todo.pop(0)) for s in free[:len(todo)]]
                if batch:
                    eng.open_many([s for s, _ in batch], [voice_state] * len(batch), [it[1] for _, it in batch],
                                  [it[2] for _, it in batch])
                    lag, delay = eng.frame_lag()
                    for s, it in batch:
                        active[s] = it
                        lead[s] = lag + delay
                B = max(active) + 1
                r = eng.step(B)
                chunks = eng.fetch_wire(B) if wire else None
                if joiner is not None:
                    chunks = list(zip(chunks, eng.fetch_flac_index(B)))
                arows = eng.fetch_align(B) if any(it[5] is not None for it in active.values()) else None
                for s in sorted(active):
                    it = active[s]
                    if not r.valid[s]:
                        if lead[s] > 0:
                            lead[s] -= 1
                            continue
                        it[4] = True
                        del active[s]
                        continue
                    lead[s] = 0
                    it[3].append(chunks[s] if wire else r.pcm[s].reshape(1, 1, FRAME).copy())
                    if it[5] is not None:
                        it[5]["rows"].append(arows[s])
                        it[5]["frames"] += 1
                        it[5]["units"] += self._units(it[3][-1], it[5]["encoding"])
                    if r.last[s]:
                        it[4] = True
                        del active[s]
        finally:
            if active:  # closed early (or failed): the rows still held stop now, without a drain
                eng.cancel_slots(sorted(active))

    def generate_parallel(self, text: str, voice_state: Voice, pauses: bool = False, rows: int | None = None,
                          sample_rate: int | None = None, encoding=None, speed: float | None = None,
                          pitch: float | None = None, timestamps: bool = False):
        """generate (pauses=False) or generate_with_pauses (pauses=True) with the text's segments on
        parallel rows: the concatenation of generate_stream_parallel's items (encoding "flac": behind
        the stream header with the true sample count, a complete file). The name is the
        reference's own: its generate_parallel (tts_model.rs:705-854) is commented out there, "for
        future exploration with GPU acceleration".
        timestamps=True (a model loaded with align=True): returns (audio, words); each segment's words
        are offset by the samples delivered before it, pauses included."""
        out = OutputOptions.of(sample_rate, encoding, speed, pitch)
        joiner = self._joiner(out)
        if timestamps and joiner is not None:
            raise ValueError("timestamps: not with flac (ask for pcm_s16le and encode the result)")
        if timestamps and not self.engine.align_enabled:
            raise ValueError("timestamps need a model loaded with align=True")
        timed = [] if timestamps else None
        chunks = list(self._stream_parallel(text, voice_state, pauses, rows, out, timed, joiner))
        if not chunks:
            raise RuntimeError("No audio generated")
        audio = b"".join(chunks) if out.wire else np.concatenate(chunks, axis=2)[0]
        if joiner is not None:  # a complete file (section 21.5)
            audio = flac_stream_header(joiner.rate, joiner.total) + audio
        if timestamps:
            rate = out.wire[0] if out.wire else SAMPLE_RATE
            words, at = [], 0
            for rec in timed:
                if rec[0] == "pause":
                    at += rec[1]
                    continue
                _, ids, params, fae, meta = rec
                for w in self._words_of(ids, meta["rows"], meta["frames"], params.max_frames, fae, out.speed,
                                        meta["units"] / rate):
                    words.append({"word": w["word"], "start": round(w["start"] + at / rate, 6),
                                  "end": round(w["end"] + at / rate, 6)})
                at += meta["units"]
            return audio, words
        return audio
