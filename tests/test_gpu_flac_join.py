"""FLAC for multi-segment responses on the GPU: the frame index the FLAC
stage writes beside each chunk (ptts_fetch_flac_index), the seam with the index
(ptts_flac_encode_ex), TTSModel's multi-segment calls with encoding="flac" against the same calls
with pcm_s16le, and the plans of engines without the stage against the parent commit's
(tests/golden/plan_ops_before_flac_index.json, written by the parent's library).

Small engines: 4 slots, synthetic weights, temp 0; six frames a row, pipelined with frame-pair
passes. The TTSModel texts run with eos_threshold -1e9 (EOS at frame 0: 4, 6 and 6 frames for the three segments)."""

import json
from pathlib import Path

import numpy as np
import pytest

import flac_decode as fd
from test_gpu_wire import make_voice
from test_text_frontend import synthetic_tokenizer

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "plan_ops_before_flac_index.json"
INF = float("inf")
FRAMES = 6
# (sample_rate, encoding, speed, volume_db): one frame per chunk; chunks of two and three frames; the
# level stage's short first chunk and long last chunk; a row that is not FLAC
ROWS = [(24000, "flac", None, None), (48000, "flac", 0.5, None), (8000, "flac", None, 6.0), (24000, "pcm_s16le", None, None)]
# two sentence chunks with no pause between them, a pause, a third chunk
TEXT = "hello world good day. world hello day good. fine day hello world. good hello fine world. [pause:200ms] hello"


def engine(**kw):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=4, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=True, back_frames=2,
                     wire=True, **kw)


def test_every_chunk_comes_with_its_frame_index():
    from pocket_tts_amd import GenerationParams
    from pocket_tts_amd.audio import flac_frames

    eng = engine(tempo=True, level=True, flac=True)
    try:
        voice = make_voice(eng)
        rng = np.random.default_rng(5)
        ps = []
        for rate, enc, speed, vol in ROWS:
            p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=FRAMES, seed=1)
            p.sample_rate, p.encoding, p.speed, p.volume_db = rate, enc, speed, vol
            ps.append(p)
        eng.open_many([0, 1, 2, 3], [voice] * 4, [rng.integers(0, 4000, size=3 + b).astype(np.int32) for b in range(4)], ps)
        got, at, shapes, started, call = [0] * 4, [0] * 4, [[] for _ in range(4)], 0, 0
        s16_bytes, delay = 0, eng.frame_lag()[1]
        while any(g < FRAMES for g in got):
            assert call < 32, "the rows never finished"
            if started >= FRAMES:  # as test_gpu_wire.drive: flush once no row has a frame left to start
                eng.flush_async(4)
            else:
                eng.step_async(4)
                started += call >= delay  # rows admitted inside a pass start at the next
            r = eng.fetch(4)
            wire, index = eng.fetch_wire(4), eng.fetch_flac_index(4)
            assert len(index) == 4
            for b, (rate, enc, _, _) in enumerate(ROWS):
                if not r.valid[b] or enc != "flac":  # an empty slot, or a row that is not FLAC: no frames
                    assert index[b] == [], (call, b, index[b])
                    assert r.valid[b] or wire[b] == b""
                    s16_bytes += len(wire[b])
                    got[b] += bool(r.valid[b])
                    continue
                got[b] += 1
                chunk, idx = wire[b], index[b]
                assert sum(n for n, _ in idx) == len(chunk), (call, b, idx, len(chunk))
                assert (len(idx) == 0) == (len(chunk) == 0) and len(idx) <= 3
                off, parts = 0, []
                for size, bs in idx:
                    assert chunk[off:off + 2] == b"\xff\xf9", (call, b, off)
                    s, first, n, used = fd.decode_frame(chunk[off:off + size], 0, rate)  # the frame decodes alone
                    assert (n, used) == (bs, size) and first == at[b] + sum(map(len, parts)), (call, b, idx)
                    parts.append(s)
                    off += size
                assert [bs for _, bs in idx[:-1]] == [4608] * (len(idx) - 1)
                if parts:
                    s = np.concatenate(parts)
                    assert chunk == flac_frames(s.astype(np.int16), at[b], rate), (call, b)
                    at[b] += s.size
                shapes[b].append([bs for _, bs in idx])
            call += 1
        assert s16_bytes == 2 * FRAMES * 1920
        assert shapes[0] == [[1920]] * FRAMES
        assert {len(x) for x in shapes[1]} >= {2, 3} and at[1] > 2 * (FRAMES - 1) * 3840  # half speed at 48 kHz
        sizes = [sum(x) for x in shapes[2]]  # the level stage holds 126 samples back until the last frame
        assert sum(sizes) == at[2] and sizes[0] < 640 < sizes[-1] and len(sizes) == FRAMES
        print("frames per chunk:", [[len(x) for x in row] for row in shapes[:3]], "level row chunk samples:", sizes)
    finally:
        eng.close()


def test_seam_with_the_index():
    from pocket_tts_amd.audio import flac_frames_index

    eng = engine(flac=True)
    plain = engine()
    try:
        s = np.random.default_rng(11477).integers(-32768, 32768, 11477).astype(np.int16)
        data, index = eng.flac_encode(s, 44100, 12345, index=True)
        assert data == eng.flac_encode(s, 44100, 12345)
        assert [bs for _, bs in index] == [4608, 4608, 2261] and sum(n for n, _ in index) == len(data)
        assert (data, index) == flac_frames_index(s, 12345, 44100)
        data, index = eng.flac_encode(s[:17], 8000, 0, index=True)
        assert index == [(len(data), 17)]
        import pocket_tts_amd as pt
        with pytest.raises(pt.PocketTTSError) as e:  # an engine without the stage has no index
            plain.fetch_flac_index(1)
        assert e.value.code == 1
    finally:
        eng.close()
        plain.close()


def model(**kw):
    import pocket_tts_amd as pt

    return pt.TTSModel.load_with_params(tokenizer=synthetic_tokenizer(), max_ctx=256, temp=0.0, eos_threshold=-1e9,
                                        wire=True, flac=True, **kw)


def prompt():
    return (0.11 * np.random.default_rng(5).standard_normal((6, 1024))).astype(np.float32)


def decoded(data, rate=24000):
    """a complete file -> its samples; the header states their number"""
    h, s, info = fd.decode_stream(data)  # (asserts the sample numbers contiguous from 0)
    assert h["rate"] == rate and h["total"] == s.size
    return s, info


def test_parallel_rows_and_pauses_are_one_stream():
    from pocket_tts_amd.audio import flac_stream_header

    m = model(max_slots=4, pipeline=True, back_frames=2)
    try:
        v = m.get_voice_state_from_prompt_tensor(prompt())
        want = np.frombuffer(m.generate_parallel(TEXT, v, pauses=True, encoding="pcm_s16le"), "<i2")
        got, info = decoded(m.generate_parallel(TEXT, v, pauses=True, encoding="flac"))
        assert np.array_equal(got, want)
        assert want.size == (4 + 6 + 6) * 1920 + 4800 and [n for _, n, _ in info] == [1920] * 10 + [4608, 192] + [1920] * 6
        # the stream: the same frames behind the header with total 0, and at another rate
        items = list(m.generate_stream_parallel(TEXT, v, pauses=True, encoding="flac", rows=2))
        assert flac_stream_header(24000, want.size) + b"".join(items) == m.generate_parallel(TEXT, v, pauses=True, encoding="flac")
        want = np.frombuffer(m.generate_parallel(TEXT, v, pauses=True, sample_rate=8000, encoding="pcm_s16le"), "<i2")
        got, _ = decoded(m.generate_parallel(TEXT, v, pauses=True, sample_rate=8000, encoding="flac"), 8000)
        assert np.array_equal(got, want)
        with pytest.raises(ValueError, match="flac"):
            m.generate_parallel(TEXT, v, pauses=True, encoding="flac", timestamps=True)
    finally:
        m.engine.close()


def test_sequential_segments_and_continuity_are_one_stream():
    from pocket_tts_amd.audio import FlacJoiner, flac_stream_header

    m = model(max_slots=1)
    try:
        v = m.get_voice_state_from_prompt_tensor(prompt())
        text = TEXT.split(" [pause")[0]  # two sentence chunks
        want = np.frombuffer(m.generate(text, v, encoding="pcm_s16le"), "<i2")
        got, _ = decoded(m.generate(text, v, encoding="flac"))
        assert want.size == (4 + 6) * 1920 and np.array_equal(got, want)
        for continuity in (False, True):
            want = np.frombuffer(m.generate_with_pauses(TEXT, v, continuity, encoding="pcm_s16le"), "<i2")
            items = list(m.generate_stream_long(TEXT, v, continuity, encoding="flac"))
            got, _ = decoded(flac_stream_header(24000, want.size) + b"".join(items))
            assert want.size == (4 + 6 + 6) * 1920 + 4800 and np.array_equal(got, want), continuity
            assert m.generate_with_pauses(TEXT, v, continuity, encoding="flac") == flac_stream_header(24000, want.size) + b"".join(items)
        a, b = "hello world good day.", "fine day hello world."
        pa, link = m.generate_continued(a, v, encoding="pcm_s16le")
        pb, _ = m.generate_continued(b, v, link, encoding="pcm_s16le")
        j = FlacJoiner(24000)
        fa, link = m.generate_continued(a, v, encoding="flac", joiner=j)
        fb, _ = m.generate_continued(b, v, link, encoding="flac", joiner=j)
        got, _ = decoded(flac_stream_header(24000, j.total) + fa + fb)
        assert np.array_equal(got, np.frombuffer(pa + pb, "<i2"))
    finally:
        m.engine.close()


def test_plan_of_an_engine_without_the_stage_is_the_parents():
    """Engine.plan_ops(8) of engines that do not enable the FLAC stage: the text the parent commit
    returns (the fixture was written by the parent's library). The FLAC engine's ops are the parent's
    too: the index is a few stores of the `flac` launch and rides in the copy of the byte counts."""
    import pocket_tts_amd as pt

    want = json.loads(GOLDEN.read_text())
    kinds = {"sequential": dict(pipeline=False),
             "pipelined_pair": dict(pipeline=True, back_frames=2),
             "pipelined_four_wire_tempo": dict(pipeline=True, back_frames=4, wire=True, tempo=True),
             "pipelined_four_wire_tempo_pitch_level": dict(pipeline=True, back_frames=4, wire=True, tempo=True,
                                                           pitch=True, level=True),
             "pipelined_four_wire_tempo_pitch_flac": dict(pipeline=True, back_frames=4, wire=True, tempo=True,
                                                          pitch=True, flac=True)}
    assert sorted(want) == sorted(kinds)
    assert sum("flac" not in kw for kw in kinds.values()) == 4
    for name, kw in kinds.items():
        eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, **kw)
        try:
            assert eng.plan_ops(8) == want[name], name
        finally:
            eng.close()
