"""Word timestamps on the host (pocket_tts_amd/align.py): the word spans of an
encoding, the monotonic path over planted band matrices, the frame -> seconds rule, and the ABI's
struct growth. No GPU."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from pocket_tts_amd import align
from pocket_tts_amd._lib import ALIGN_TOKENS, SlotOpts4, SlotOpts5
from pocket_tts_amd.text import load_tokenizer, prepare_text_prompt

TOKENIZER = Path(__file__).parent / "golden" / "reference_tokenizer.json"


@pytest.fixture(scope="module")
def tok():
    return load_tokenizer(TOKENIZER)


def test_word_spans_join_punctuation_and_suffixes(tok):
    ids = tok(prepare_text_prompt("Hello, world! This is unbelievable."))
    spans = align.word_spans(tok, ids)
    assert [w for w, _, _ in spans] == ["Hello,", "world!", "This", "is", "unbelievable."]
    # the spans tile the encoding, the leading special token with the first word
    assert spans[0][1] == 0 and spans[-1][2] == len(ids)
    assert all(a[2] == b[1] for a, b in zip(spans, spans[1:]))
    pieces = tok.pieces(ids)
    for _, j0, j1 in spans[1:]:
        assert pieces[j0].startswith(align.META) and not any(p.startswith(align.META) for p in pieces[j0 + 1:j1])


def test_word_spans_single_word(tok):
    ids = tok(prepare_text_prompt("Hello"))  # padded with spaces in front: bare metaspace pieces
    spans = align.word_spans(tok, ids)
    assert len(spans) == 1 and spans[0][0].startswith("Hello") and spans[0][1:] == (0, len(ids))


def band(frames, bounds, leak=0.1):
    """W [frames][words]: frame t puts 1 - leak on the word whose planted range holds t, and leak
    spread uniformly over all words. bounds[w] = first frame of word w (ascending, bounds[0] = 0)."""
    n = len(bounds)
    W = np.full((frames, n), leak / n)
    for t in range(frames):
        w = max(i for i in range(n) if bounds[i] <= t)
        W[t, w] += 1.0 - leak
    return W


@pytest.mark.parametrize("frames,bounds", [
    (1, [0]),
    (3, [0, 1, 2, 3, 4]),  # fewer frames than words: the path reaches words 0, 1, 2
    (12, [0, 2, 7, 8]),
    (40, [0, 3, 4, 9, 17, 18, 25, 31, 39]),
])
def test_monotonic_path_recovers_planted_boundaries(frames, bounds):
    W = band(frames, bounds)
    path = align.monotonic_path(W)
    want = [max(i for i in range(len(bounds)) if bounds[i] <= t) for t in range(frames)]
    assert path == want
    assert path[0] == 0 and all(0 <= b - a <= 1 for a, b in zip(path, path[1:]))


def test_monotonic_path_ties_go_to_the_smaller_word():
    assert align.monotonic_path(np.full((3, 5), 0.2)) == [0, 0, 0]  # every path scores the same
    # frame 1 cannot tell words 0 and 1 apart: the path stays on word 0 there and moves at frame 2
    W = np.array([[0.8, 0.1, 0.1], [0.45, 0.45, 0.1], [0.1, 0.8, 0.1], [0.1, 0.1, 0.8]])
    assert align.monotonic_path(W) == [0, 0, 1, 2]
    assert align.monotonic_path(np.zeros((0, 3))) == [] and align.monotonic_path(np.zeros((2, 0))) == []
    # values under the floor count as the floor: no -inf, the constraint c(0) = 0 holds
    assert align.monotonic_path(np.array([[0.0, 1.0], [0.0, 1.0]])) == [0, 1]


def test_word_matrix_sums_a_words_tokens():
    A = np.arange(12, dtype=np.float64).reshape(2, 6)
    W = align.word_matrix(A, [("a", 0, 2), ("b", 2, 3), ("c", 3, 6)])
    assert W.tolist() == [[1, 2, 12], [13, 8, 30]]


SPANS = [("one", 0, 1), ("two", 1, 3), ("three", 3, 4), ("four", 4, 5)]


def test_word_times_speed_and_eos():
    path = [0, 0, 1, 1, 1, 2, 2, 2, 2, 2]  # word 3 is never reached
    w = align.word_times(path, SPANS, speed=1.0)
    assert [x["word"] for x in w] == ["one", "two", "three", "four"]
    assert [x["start"] for x in w] == pytest.approx([0.0, 0.16, 0.40, 0.80])
    assert [x["end"] for x in w] == pytest.approx([0.16, 0.40, 0.80, 0.80])  # unreached: start = end = the end
    half = align.word_times(path, SPANS, speed=0.5)
    assert [x["start"] for x in half] == pytest.approx([0.0, 0.32, 0.80, 1.60])
    fast = align.word_times(path, SPANS, speed=2.0, total_seconds=0.4)
    assert [x["start"] for x in fast] == pytest.approx([0.0, 0.08, 0.20, 0.40])
    assert fast[-1]["end"] == pytest.approx(0.40)
    # the row stopped by EOS at frame 7: the last word ends there, not at the end of the audio
    spans3, p3 = SPANS[:3], path
    e = align.word_times(p3, spans3, speed=1.0, eos_frame=7, total_seconds=0.8)
    assert e[-1]["start"] == pytest.approx(0.40) and e[-1]["end"] == pytest.approx(0.56)
    e2 = align.word_times(p3, spans3, speed=2.0, eos_frame=7, total_seconds=0.4)
    assert e2[-1]["end"] == pytest.approx(0.28)
    assert align.word_times(p3, spans3, speed=1.0)[-1]["end"] == pytest.approx(0.80)  # no EOS: the audio's end
    for x in w + half + fast + e:
        assert x["start"] <= x["end"]


def test_diagonality_orders_band_flat_and_stuck():
    n = 8
    diag = np.eye(n)[np.repeat(np.arange(n), 3)]  # 24 frames walking 8 tokens
    flat = np.full((24, n), 1.0 / n)
    stuck = np.zeros((24, n))
    stuck[:, 0] = 1.0
    d, f, s = align.diagonality(diag), align.diagonality(flat), align.diagonality(stuck)
    assert d == pytest.approx(1.0) and f <= 1.0 / n + 1e-12 and s == pytest.approx(1.0 / n)
    assert 0.0 <= min(d, f, s) and align.diagonality(np.zeros((0, 0))) == 0.0
    assert align.diagonality(band(40, [0, 3, 4, 9, 17, 18, 25, 31, 39])) > 0.85


def test_timestamps_end_to_end_on_planted_rows(tok):
    ids = tok(prepare_text_prompt("Hello, world! This is unbelievable."))
    spans = align.word_spans(tok, ids)
    firsts = [0, 4, 9, 11, 15]
    A = np.full((20, len(ids)), 0.1 / len(ids))
    for t in range(20):
        w = max(i for i in range(5) if firsts[i] <= t)
        A[t, spans[w][1]:spans[w][2]] += 0.9 / (spans[w][2] - spans[w][1])
    words = align.timestamps(tok, ids, A, speed=1.0, eos_frame=17, total_seconds=1.6)
    assert [w["word"] for w in words] == [s[0] for s in spans]
    assert [w["start"] for w in words] == pytest.approx([0.08 * f for f in firsts])
    assert words[-1]["end"] == pytest.approx(0.08 * 17)


def test_slot_opts_grows_to_64_bytes():
    """The 56-byte struct keeps its layout (a caller built before `align` states 56 and its rows are
    read with align = 0); `align` lies at offset 56."""
    assert C.sizeof(SlotOpts4) == 56 and C.sizeof(SlotOpts5) == 64
    assert SlotOpts5.align.offset == 56 and SlotOpts5.reserved2.offset == 60
    for name, _ in SlotOpts4._fields_:
        assert getattr(SlotOpts4, name).offset == getattr(SlotOpts5, name).offset, name
    assert ALIGN_TOKENS == 128
    header = (Path(__file__).parents[1] / "include" / "pocket_tts.h").read_text()
    assert "#define PTTS_ALIGN_TOKENS 128" in header and "#define PTTS_ABI_VERSION 6" in header
    assert header.index("int limit;") < header.index("int align;") < header.index("int reserved2;")


# ---------------------------------------------------------------------------------------------
# the server's routes, on the stand-in engine of serve.py (a planted band per frame)
# ---------------------------------------------------------------------------------------------
def service(align_stage=True, **kw):
    from types import SimpleNamespace

    from pocket_tts_amd import serve

    eng = serve.StandInEngine(max_slots=4, max_ctx=10_000, align=align_stage)
    sch = serve.BatchScheduler(eng)
    svc = serve.TTSService(sch, {"alba": SimpleNamespace(n_frames=10)}, default_voice="alba",
                           tokenizer=serve.load_tokenizer(str(TOKENIZER)), **kw)
    return eng, sch, svc


def planted_words(tokenizer, text, frames, at=0.0):
    """What the stand-in's band gives for `text` as one segment of `frames` frames starting at `at` s."""
    from pocket_tts_amd.serve import stand_in_align_row

    ids = tokenizer(prepare_text_prompt(text))
    A = np.stack([stand_in_align_row(k, frames, len(ids)) for k in range(frames)])
    words = align.timestamps(tokenizer, ids, A, 1.0, None, frames * 0.08)
    return [{"word": w["word"], "start": round(w["start"] + at, 6), "end": round(w["end"] + at, 6)} for w in words]


def test_http_timestamps_json_and_the_same_audio():
    import base64

    from fastapi.testclient import TestClient

    from pocket_tts_amd.serve import create_app

    eng, sch, svc = service()
    try:
        c = TestClient(create_app(svc))
        text, nf = "Hello, world! This is unbelievable.", 12
        body = {"text": text, "max_frames": nf}
        plain = c.post("/generate", json=body)
        r = c.post("/generate", json={**body, "timestamps": True})
        assert plain.status_code == 200 and r.status_code == 200
        assert r.headers["content-type"].startswith("application/json")
        j = r.json()
        assert sorted(j) == ["audio", "content_type", "sample_rate", "words"]
        assert j["content_type"] == "audio/wav" and j["sample_rate"] == 24000
        assert base64.b64decode(j["audio"]) == plain.content  # the bytes of the same request without timestamps
        assert [sorted(w) for w in j["words"]] == [["end", "start", "word"]] * 5
        assert j["words"] == planted_words(svc.tokenizer, text, nf)
        assert [w["word"] for w in j["words"]] == ["Hello,", "world!", "This", "is", "unbelievable."]
        starts = [w["start"] for w in j["words"]]
        assert starts[0] == 0.0 and starts == sorted(starts) and j["words"][-1]["end"] == pytest.approx(nf * 0.08)
        assert eng.params_log[-1].align and not eng.params_log[-2].align
        # timestamps false / null: the request of before
        for off in (False, None):
            r = c.post("/generate", json={**body, "timestamps": off})
            assert r.content == plain.content and not eng.params_log[-1].align
        # the OpenAI route: the bytes and the content type it would have sent
        o_plain = c.post("/v1/audio/speech", json={"input": text, "response_format": "pcm"})
        o = c.post("/v1/audio/speech", json={"input": text, "response_format": "pcm", "timestamps": True})
        assert o.status_code == 200 and o.json()["content_type"] == "audio/pcm"
        assert base64.b64decode(o.json()["audio"]) == o_plain.content
        assert [w["word"] for w in o.json()["words"]] == [w["word"] for w in j["words"]]
    finally:
        sch.close()


def test_http_timestamps_long_form_offsets_are_the_pauses_samples():
    from fastapi.testclient import TestClient

    from pocket_tts_amd.serve import create_app

    eng, sch, svc = service()
    try:
        c = TestClient(create_app(svc))
        nf = 5
        r = c.post("/generate", json={"text": "Hello there [pause:500ms] General Kenobi", "max_frames": nf,
                                      "long_form": True, "timestamps": True})
        assert r.status_code == 200
        words = r.json()["words"]
        from pocket_tts_amd.serve import stand_in_align_row
        from pocket_tts_amd.text import long_form_segments, segment_request

        tok_ = svc.tokenizer
        want, at, pause = [], 0, 500 * 24000 // 1000  # samples
        segs = long_form_segments("Hello there [pause:500ms] General Kenobi", tok_.count_tokens, True)
        assert [k for k, _ in segs] == ["text", "pause", "text"] and segs[1][1] == 500
        for kind, val in segs:
            if kind == "pause":
                at += val * 24000 // 1000
                continue
            ids = segment_request(val, tok_)[0]
            A = np.stack([stand_in_align_row(k, nf, len(ids)) for k in range(nf)])
            for w in align.timestamps(tok_, ids, A, 1.0, None, nf * 0.08):
                want.append({"word": w["word"], "start": round(w["start"] + at / 24000, 6),
                             "end": round(w["end"] + at / 24000, 6)})
            at += nf * 1920
        assert [w["word"] for w in words] == ["Hello", "there.", "General", "Kenobi."]
        assert words == want
        assert words[2]["start"] - words[1]["end"] == pytest.approx(pause / 24000)
    finally:
        sch.close()


def test_http_timestamps_refusals():
    from fastapi.testclient import TestClient

    from pocket_tts_amd.serve import create_app

    eng, sch, svc = service()
    try:
        c = TestClient(create_app(svc))
        n = len(eng.params_log)
        assert c.post("/stream", json={"text": "Hello there", "timestamps": True}).status_code == 400
        assert c.post("/generate", json={"text": "Hello there. And more.", "continuity": True,
                                         "timestamps": True}).status_code == 400
        assert c.post("/generate", json={"token_ids": [3, 1, 2], "max_frames": 2, "timestamps": True}).status_code == 400
        assert c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "timestamps": True}).status_code == 400
        assert len(eng.params_log) == n  # nothing was admitted
    finally:
        sch.close()
    eng, sch, svc = service(align_stage=False)
    try:
        c = TestClient(create_app(svc))
        assert c.post("/generate", json={"text": "Hello there", "timestamps": True}).status_code == 400
        assert c.post("/v1/audio/speech", json={"input": "Hello there", "timestamps": True}).status_code == 400
        assert c.post("/generate", json={"text": "Hello there", "max_frames": 2}).status_code == 200
        assert len(eng.params_log) == 1
    finally:
        sch.close()


def test_http_timestamps_over_the_token_limit_is_a_400_and_fails_nobody_else():
    """A timestamps row of more than PTTS_ALIGN_TOKENS tokens is refused by the service (400), never by
    the engine, whose refusal would fail every request of that batched admission: a plain request
    queued beside it completes. With long_form the same text is cut into rows that fit."""
    from fastapi.testclient import TestClient

    from pocket_tts_amd import GenerationParams, serve

    eng = serve.StandInEngine(max_slots=4, max_ctx=10_000, align=True, step_s=0.002)
    sch = serve.BatchScheduler(eng)
    from types import SimpleNamespace
    svc = serve.TTSService(sch, {"alba": SimpleNamespace(n_frames=10)}, default_voice="alba",
                           tokenizer=serve.load_tokenizer(str(TOKENIZER)))
    try:
        c = TestClient(serve.create_app(svc))
        long_text = " ".join(f"sentence number {i} goes on." for i in range(40))
        assert svc._count_tokens(prepare_text_prompt(long_text)) > ALIGN_TOKENS
        other = svc.request(text="Hello there", max_frames=30)  # queued and running meanwhile
        n = len(eng.params_log)
        for route, key in (("/generate", "text"), ("/v1/audio/speech", "input")):
            r = c.post(route, json={key: long_text, "timestamps": True, "long_form": False})
            assert r.status_code == 400 and "128" in r.json()["detail"], route
        with pytest.raises(ValueError):
            svc.request(text=long_text, timestamps=True)
        assert len(eng.params_log) <= n + 1 and not any(p.align for p in eng.params_log)
        assert other.audio().size == 30 * 1920  # the other client's request is untouched
        assert c.post("/generate", json={"text": long_text, "max_frames": 2}).status_code == 200  # no timestamps: as before
        r = c.post("/generate", json={"text": long_text, "timestamps": True, "long_form": True, "max_frames": 2})
        assert r.status_code == 200 and len(r.json()["words"]) == 5 * 40
        # the stand-in refuses what the engine refuses
        p = GenerationParams(max_frames=2)
        p.align = True
        m = len(eng.admit_log)
        with pytest.raises(RuntimeError):
            eng.open_many([3], [None], [np.arange(ALIGN_TOKENS + 1)], [p])
        assert len(eng.admit_log) == m
    finally:
        sch.close()


def test_http_timestamps_with_flac_and_under_a_continuity_default():
    from types import SimpleNamespace

    from fastapi.testclient import TestClient

    from pocket_tts_amd import serve

    eng, sch, svc = service()
    try:
        c = TestClient(serve.create_app(svc))
        for route, body in (("/generate", {"text": "Hello there", "encoding": "flac"}),
                            ("/v1/audio/speech", {"input": "Hello there", "response_format": "flac"})):
            assert c.post(route, json={**body, "timestamps": True}).status_code == 400, route
        assert not eng.params_log
    finally:
        sch.close()
    eng, sch, svc = service(continuity=True)  # a server started with --continuity
    try:
        c = TestClient(serve.create_app(svc))
        r = c.post("/generate", json={"text": "Hello there", "timestamps": True})
        assert r.status_code == 400 and "continuity: false" in r.json()["detail"]
        r = c.post("/generate", json={"text": "Hello there", "timestamps": True, "continuity": False, "max_frames": 3})
        assert r.status_code == 200 and [w["word"] for w in r.json()["words"]] == ["Hello", "there."]
    finally:
        sch.close()
