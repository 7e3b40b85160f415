"""TTSModel.generate_parallel / generate_stream_parallel on the GPU: the
segments of one text as rows of one batch. Every text segment is compared with the CPU oracle's
own run of that segment (new_state, prefill(prompt), prefill_tokens(ids), step) under PCM_TOL of
conftest.py, never with another run of the engine; pauses are exact zeros of the right length at
the right places; wire bytes equal Engine.encode_wire of each segment's own f32 PCM.

Shapes: max_ctx 256, a 6-frame random prompt, the synthetic tokenizer of test_text_frontend.py.
The oracle trajectories are computed once per session and shared. eos_threshold is inf (a segment
runs its max_gen_len frames) except where a test says otherwise: there -1e9 makes EOS fire at
frame 0, so a segment has 1 + frames_after_eos frames (6 up to 4 words, else 4) and its whole
oracle trajectory costs a handful of CPU steps."""

import numpy as np
import pytest
from conftest import PCM_TOL, pcm_err
from test_gpu_parity import _noise
from test_text_frontend import synthetic_tokenizer

pytestmark = pytest.mark.gpu

INF = float("inf")
TEXT = "hello world, good day... fine [pause:250ms] hello"
TEXT_SEEDS = "hello world good day. world hello day good. fine day hello world. good hello fine world."
FRAME = 1920


def prompt():
    return (0.11 * np.random.default_rng(5).standard_normal((6, 1024))).astype(np.float32)


def model(**kw):
    import pocket_tts_amd as pt

    kw.setdefault("temp", 0.0)
    kw.setdefault("eos_threshold", INF)
    return pt.TTSModel.load_with_params(tokenizer=synthetic_tokenizer(), max_ctx=256, **kw)


def plan(text, pauses):
    """The segment list, restated from text.py's pieces: ("pause", samples) | ("text", ids, frames at
    eos inf, frames_after_eos)."""
    from pocket_tts_amd.text import (estimate_frames_after_eos, long_text_segments, max_gen_len,
                                     prepare_text_prompt, silence_samples, split_into_best_sentences)

    tok = synthetic_tokenizer()
    out = []
    for kind, val in (long_text_segments(text) if pauses else [("text", text)]):
        if kind == "pause":
            out.append(("pause", silence_samples(val, 24000)))
            continue
        for c in split_into_best_sentences(val, tok.count_tokens):
            p = prepare_text_prompt(c)
            out.append(("text", np.asarray(tok(p), np.int32), max_gen_len(p), estimate_frames_after_eos(c)))
    return out


_TRAJ = {}


def oracle_pcm(oracle, ids, n, seed=None, temp=0.0):
    """Frames 0 .. n-1 of the segment with these ids (and this seed's noise at temp > 0)."""
    key = (ids.tobytes(), seed, temp)
    if key not in _TRAJ:
        s = oracle.new_state(256)
        s.prefill(prompt())
        s.prefill_tokens(ids)
        _TRAJ[key] = (s, [], [None])
    s, frames, lat = _TRAJ[key]
    while len(frames) < n:
        o = s.step(lat[0], noise=_noise(seed, len(frames), temp, None) if temp > 0 else None)
        lat[0] = o["latent"]
        frames.append(o["pcm"].copy())
    return frames[:n]


def split_items(items, segs, n_frames):
    """The stream's items grouped by the plan: n_frames[j] frames for text segment j, then the next
    segment's items (a pause is one item of its own length, never 1920 here); nothing is left over."""
    out, i, j = [], 0, 0
    for k, seg in enumerate(segs):
        if seg[0] == "pause":
            assert seg[1] != FRAME and i < len(items) and items[i].shape == (1, 1, seg[1]), (k, i)
            assert items[i].dtype == np.float32 and not items[i].any(), k
            i += 1
            continue
        fr = items[i:i + n_frames[j]]
        assert len(fr) == n_frames[j] and all(x.shape == (1, 1, FRAME) for x in fr), (k, len(fr))
        out.append([x[0, 0] for x in fr])
        i += n_frames[j]
        j += 1
    assert i == len(items), (i, len(items))
    return out


def check_against_oracle(oracle, items, segs, n_frames=None, seeds=None, temp=0.0, tol=PCM_TOL, tag=""):
    """n_frames: frames per text segment (default: its max_gen_len, eos inf)."""
    text = [s for s in segs if s[0] == "text"]
    n_frames = n_frames or [s[2] for s in text]
    got = split_items(items, segs, n_frames)
    worst = 0.0
    for j, (seg, fr) in enumerate(zip(text, got)):
        assert len(fr) == n_frames[j], (tag, j, len(fr), n_frames[j])
        ref = oracle_pcm(oracle, seg[1], n_frames[j], seeds[j] if seeds else None, temp)
        for i, (a, b) in enumerate(zip(fr, ref)):
            e = pcm_err(a - b)
            worst = max(worst, e)
            assert e <= tol, (tag, j, i, e)
    print(f"{tag}: {len(text)} segments, {sum(n_frames)} frames, worst PCM error {worst:.3g}")
    return got


@pytest.mark.parametrize("kw,rows", [({}, None), ({}, 2), ({"pipeline": True, "back_frames": 2}, None)],
                         ids=["rows4", "rows2-refill", "pipelined-bf2"])
def test_generate_parallel_matches_oracle(oracle, kw, rows):
    """Four text segments and three pauses on a 4-slot engine: all rows at once, two rows refilled
    as segments end, and on a pipelined engine with frame-pair passes (frame_lag handling)."""
    segs = plan(TEXT, True)
    assert [s[0] for s in segs] == ["text", "pause", "text", "pause", "text", "pause", "text"]
    assert [s[2] for s in segs if s[0] == "text"] == [52, 52, 39, 39] and [s[1] for s in segs if s[0] == "pause"] == [
        4800, 12000, 6000]
    m = model(max_slots=4, **kw)
    try:
        v = m.get_voice_state_from_prompt_tensor(prompt())
        items = list(m.generate_stream_parallel(TEXT, v, pauses=True, rows=rows))
        check_against_oracle(oracle, items, segs, tag=f"{kw} rows={rows}")
        audio = m.generate_parallel(TEXT, v, pauses=True, rows=rows)
        assert audio.shape == (1, 182 * FRAME + 22800)
        assert np.array_equal(audio[0], np.concatenate([x[0, 0] for x in items]))  # temp 0: seeds do not matter
        assert m._seed == 8  # one per text segment and call
    finally:
        m.engine.close()


def test_parallel_equals_sequential_at_temp(oracle):
    """temp 0.7, eos_threshold -1e9 (EOS at frame 0: 4 and 6 frames): generate_parallel and
    generate from the same _seed have the same frame counts, each side within PCM_TOL of the
    oracle run with the same seeds' noise, hence within 2 PCM_TOL of each other."""
    segs = plan(TEXT_SEEDS, False)
    assert len(segs) == 2 and [s[3] for s in segs] == [3, 5]
    n_frames = [1 + s[3] for s in segs]
    m = model(temp=0.7, eos_threshold=-1e9, max_slots=4)
    try:
        v = m.get_voice_state_from_prompt_tensor(prompt())
        m._seed = 40
        par = m.generate_parallel(TEXT_SEEDS, v)
        assert m._seed == 42
        m._seed = 40
        seq = m.generate(TEXT_SEEDS, v)
        assert par.shape == seq.shape == (1, sum(n_frames) * FRAME)
        for name, x in (("parallel", par), ("sequential", seq)):
            items = [x[:, None, i * FRAME:(i + 1) * FRAME] for i in range(sum(n_frames))]
            check_against_oracle(oracle, items, segs, n_frames, seeds=[41, 42], temp=0.7, tag=name)
        d = pcm_err(par - seq)
        print(f"parallel vs sequential: {d:.3g}")
        assert d <= 2 * PCM_TOL
    finally:
        m.engine.close()


def test_wide_batch_of_twenty_segments(oracle):
    """20 one-word segments on 20 rows (the back part's >= 16-row matrix-core path), eos_threshold
    -1e9: 6 frames each, all checked (the first 3 and the last among them)."""
    text = ", ".join("abcdefghijklmnopqrst")
    segs = plan(text, True)
    assert sum(s[0] == "text" for s in segs) == 20 and sum(s[0] == "pause" for s in segs) == 19
    m = model(eos_threshold=-1e9, max_slots=20)
    try:
        v = m.get_voice_state_from_prompt_tensor(prompt())
        items = list(m.generate_stream_parallel(text, v, pauses=True))
        check_against_oracle(oracle, items, segs, [6] * 20, tag="wide")
    finally:
        m.engine.close()


def test_parallel_wire_bytes(oracle):
    """8 kHz mu-law: the bytes are, segment by segment, Engine.encode_wire of that segment's f32 PCM
    from a run without a format (each segment is resampled on its own), with audio.py's encoded
    silence for the pauses; closing the generator early cancels the rows it holds."""
    from pocket_tts_amd.audio import wire_bytes

    segs = plan(TEXT, True)
    m = model(max_slots=4, wire=True, pipeline=True, back_frames=2)
    try:
        v = m.get_voice_state_from_prompt_tensor(prompt())
        items = list(m.generate_stream_parallel(TEXT, v, pauses=True))
        pcm = check_against_oracle(oracle, items, segs, tag="wire model, no format")
        got = m.generate_parallel(TEXT, v, pauses=True, sample_rate=8000, encoding="ulaw")
        want, j = [], 0
        for s in segs:
            if s[0] == "pause":
                want.append(wire_bytes(np.zeros(s[1] // 3, np.float32), "ulaw"))
            else:
                want.append(m.engine.encode_wire(np.concatenate(pcm[j]), 8000, "ulaw"))
                j += 1
        assert isinstance(got, bytes) and got == b"".join(want)
        # early close: the four rows are cancelled without a drain, and the engine is reusable at once
        it = m.generate_stream_parallel(TEXT, v, pauses=True)
        first = [next(it) for _ in range(3)]
        it.close()
        r = m.engine.step(4)
        assert not r.valid.any()
        again = list(m.generate_stream_parallel(TEXT, v, pauses=True))
        assert all(np.array_equal(a, b) for a, b in zip(first, again[:3]))
        assert len(again) == len(items) and all(np.array_equal(a, b) for a, b in zip(again, items))
    finally:
        m.engine.close()
