"""Continuity chains on the CPU: the scheduler runs the sentence chunks of a
continuity request one after another on one slot, each admit_log with the concatenated ids, its
predecessor's delivered latents as a teacher-forced prefix and keep_codec. Driven by the stand-in
engine of serve.py, which records what every admission is given; the real-engine rule is
tests/test_gpu_continuation.py."""

from types import SimpleNamespace

import numpy as np
import pytest
from test_longform import VOICE, expected_segments
from test_text_frontend import synthetic_tokenizer

from pocket_tts_amd import TTSModel
from pocket_tts_amd.audio import pcm_i16_le_bytes
from pocket_tts_amd.serve import BatchScheduler, RequestGroup, StandInEngine, TTSService, create_app
from pocket_tts_amd.text import silence_samples

# several sentence chunks before the pause and several after it; every chunk is one utterance
TEXT = ("The quick brown fox jumps over the lazy dog near the quiet river bank today. "
        "A second sentence follows the first one with a few more words to fill its chunk up. "
        "And a third sentence closes the first piece of this long text for good. [pause:300ms] "
        "After the pause a new chain starts with this rather long sentence about nothing at all. "
        "Its successor continues it and ends the text.")


def service(eng, **kw):
    sch = BatchScheduler(eng, segment_rows=4)
    return sch, TTSService(sch, {"v": VOICE}, default_voice="v", tokenizer=synthetic_tokenizer(), temp=0.0,
                           eos_threshold=float("inf"), **kw)


def lat_of(adm, n):
    """The stand-in's latents of the n frames of admission number adm."""
    return np.array([[adm * 1000 + k] * 32 for k in range(n)], np.float32)


def check_chain(admit_log, want, frames, ctx=10**9):
    """admit_log: the stand-in's record; want: expected_segments of the text; frames: frames each text
    segment generates. One chain per run of text segments; each link on its predecessor's slot, with
    both segments' ids, the predecessor's latents and keep_codec - or, where that exceeds ctx, plain.
    Returns the keep_codec flags."""
    texts = [w for w in want if w[0] == "text"]
    assert len(admit_log) == len(texts)
    prev = None  # (index, ids) of the predecessor in the chain
    k = 0
    for w in want:
        if w[0] == "pause":
            prev = None
            continue
        slot, ids, pre, keep = admit_log[k]
        if prev is None or VOICE.n_frames + len(prev[1]) + len(w[1]) + 2 * frames > ctx:
            assert ids == w[1] and pre is None and not keep, k
        else:
            assert slot == admit_log[prev[0]][0], k
            assert ids == prev[1] + w[1] and keep, k
            np.testing.assert_array_equal(pre, lat_of(prev[0], frames))
        prev = (k, w[1])
        k += 1
    return [a[3] for a in admit_log]


def kinds(want):
    """The text's shape: at least two links before its one pause and two after it."""
    k = [w[0] for w in want]
    i = k.index("pause")
    assert k.count("pause") == 1 and i >= 2 and len(k) - i - 1 >= 2, k
    return i, len(k) - i - 1


def test_chain_runs_on_one_slot_in_order():
    """A continuity request's segments are admit_log strictly one after another (each admission of
    one row, the next only after its predecessor's last frame), every link on the slot its
    predecessor used, with the concatenated ids, exactly the predecessor's delivered latents and
    keep_codec; a pause restarts the chain; only the new frames are streamed."""
    eng = StandInEngine(max_slots=4, max_ctx=10_000)
    sch, svc = service(eng)
    try:
        want = expected_segments(TEXT, synthetic_tokenizer())
        a, b = kinds(want)
        g = svc.request(text=TEXT, continuity=True, max_frames=6)
        assert isinstance(g, RequestGroup) and g.continuity and g.rows == 1
        items = list(g.stream(timeout=30))
        keep = check_chain(eng.admit_log, want, 6)
        assert keep == [False] + [True] * (a - 1) + [False] + [True] * (b - 1)
        sizes = [x.size for x in items]
        assert sizes == [1920] * (6 * a) + [silence_samples(300, 24000)] + [1920] * (6 * b)
        assert sch.load() == 0 and not sch.active and not sch.waiting and not sch.handoff
    finally:
        sch.close()


def test_overflowing_chunk_is_admitted_plain():
    """Where voice + both chunks' ids + the prefix + max_frames would exceed max_ctx, the chunk is a
    plain segment: its own ids, no prefix, no keep_codec."""
    tok = synthetic_tokenizer()
    want = expected_segments(TEXT, tok)
    frames = 6
    pairs = sorted(len(u[1]) + len(w[1]) for u, w in zip(want, want[1:]) if u[0] == w[0] == "text")
    ctx = VOICE.n_frames + pairs[len(pairs) // 2] + 2 * frames - 1  # room for some links, not for all
    eng = StandInEngine(max_slots=2, max_ctx=ctx)
    sch, svc = service(eng)
    try:
        g = svc.request(text=TEXT, continuity=True, max_frames=frames)
        n_text = sum(w[0] == "text" for w in want)
        assert len(list(g.stream(timeout=30))) == n_text * frames + 1
        keep = check_chain(eng.admit_log, want, frames, ctx)
        assert any(keep) and keep.count(False) > 2, keep  # (2: the two chains' first links)
    finally:
        sch.close()


def test_cancel_mid_chain():
    """Cancel while the second link runs: its slot is freed, no successor is admit_log."""
    eng = StandInEngine(max_slots=2, max_ctx=100_000)
    sch, svc = service(eng)
    try:
        g = svc.request(text=TEXT, continuity=True, max_frames=40)
        it = g.stream(timeout=30)
        for _ in range(45):  # into the second link
            next(it)
        g.cancel()
        sch.call(lambda: None)
        list(it)
        assert len(eng.admit_log) == 2 and eng.admit_log[1][3]
        assert sch.load() == 0 and not sch.active and not sch.waiting and not sch.handoff and not g.pending
        assert eng.cancelled[-1] == [eng.admit_log[1][0]]
        nxt = sch.submit([9, 7], VOICE, SimpleNamespace(max_frames=3))
        assert len(list(nxt.stream(timeout=30))) == 3 and nxt.slot == 0
        assert eng.admit_log[2][2] is None and not eng.admit_log[2][3]
    finally:
        sch.close()


def test_routes_and_defaults():
    """`continuity` with token_ids is 400; the three audio routes take it; the server default
    (--continuity) is off, and a request without it is scheduled exactly as before: the same
    admissions (slots, ids, no prefix, no keep_codec) and the same bytes."""
    from fastapi.testclient import TestClient

    def run(body, **kw):
        eng = StandInEngine(max_slots=4, max_ctx=10_000)
        sch, svc = service(eng, **kw)
        try:
            r = TestClient(create_app(svc)).post("/stream", json=body)
            return r, [(s, ids, None if p is None else p.tolist(), k) for s, ids, p, k in eng.admit_log]
        finally:
            sch.close()

    body = {"text": TEXT, "long_form": True, "max_frames": 4}
    base, adm = run(body)
    assert base.status_code == 200 and all(p is None and not k for _, _, p, k in adm)
    assert len({s for s, _, _, _ in adm}) > 1  # parallel rows
    off, adm_off = run({**body, "continuity": False})
    assert off.content == base.content and adm_off == adm
    on, adm_on = run({"text": TEXT, "continuity": True, "max_frames": 4})
    assert on.status_code == 200 and len(on.content) == len(base.content)
    a, b = kinds(expected_segments(TEXT, synthetic_tokenizer()))
    assert [k for _, _, _, k in adm_on] == [False] + [True] * (a - 1) + [False] + [True] * (b - 1)
    dflt, adm_dflt = run({"text": TEXT, "max_frames": 4}, continuity=True)  # the server's default
    assert adm_dflt == adm_on and dflt.content == on.content
    plain, adm_plain = run({"text": "Hello world"})
    assert len(adm_plain) == 1 and adm_plain[0][2] is None and not adm_plain[0][3]

    eng = StandInEngine(max_slots=4, max_ctx=10_000)
    sch, svc = service(eng)
    try:
        c = TestClient(create_app(svc))
        for route, key in (("/generate", "text"), ("/stream", "text"), ("/v1/audio/speech", "input")):
            bad = {"token_ids": [3, 1], "words": 1, "continuity": True}
            assert c.post(route, json=bad).status_code == 400, route
            n0 = len(eng.admit_log)
            ok = c.post(route, json={key: "One sentence here. And another one there.", "continuity": True})
            assert ok.status_code == 200, route
            assert all(a[0] == eng.admit_log[n0][0] for a in eng.admit_log[n0:])
        assert c.post("/generate", json={"token_ids": [3, 1], "words": 1, "continuity": False}).status_code == 200
    finally:
        sch.close()


class OneSlot(StandInEngine):
    """The stand-in behind the calls TTSModel makes (open / step on row 0, a frame lag of one call)."""

    max_lsd_steps = 1

    def open(self, slot, voice, ids, params):
        self.open_many([slot], [voice], [ids], [params])

    def frame_lag(self):
        return 1, 0

    def step(self, n):
        self.step_async(n)
        return self.fetch(n)


@pytest.mark.parametrize("continuity", [False, True])
def test_tts_model_drives_the_same_sequence(continuity):
    """TTSModel.generate_stream_long(continuity=True) on a one-slot engine: the admissions the
    scheduler makes for the same text; without the flag, plain segments as before."""
    tok = synthetic_tokenizer()
    want = expected_segments(TEXT, tok)
    eng = OneSlot(max_slots=1, max_ctx=10_000)
    m = TTSModel(eng, temp=0.0, lsd_decode_steps=1, eos_threshold=float("inf"), noise_clamp=None, tokenizer=tok)
    items = list(m.generate_stream_long(TEXT, VOICE, continuity=continuity))
    texts = [w for w in want if w[0] == "text"]
    assert sum(x.shape[2] for x in items) == sum(w[2] for w in texts) * 1920 + silence_samples(300, 24000)
    if not continuity:
        assert [(ids, p, k) for _, ids, p, k in eng.admit_log] == [(w[1], None, False) for w in texts]
        return
    assert len(eng.admit_log) == len(texts) and all(a[0] == 0 for a in eng.admit_log)
    prev, k = None, 0
    for w in want:
        if w[0] == "pause":
            prev = None
            continue
        _, ids, pre, keep = eng.admit_log[k]
        if prev is None:
            assert ids == w[1] and pre is None and not keep
        else:
            assert ids == prev[1] + w[1] and keep
            np.testing.assert_array_equal(pre, lat_of(prev[0], prev[2]))
        prev = (k, w[1], w[2])
        k += 1
    # one link at a time through generate_continued
    eng2 = OneSlot(max_slots=1, max_ctx=10_000)
    m2 = TTSModel(eng2, temp=0.0, lsd_decode_steps=1, eos_threshold=float("inf"), noise_clamp=None, tokenizer=tok)
    pcm_a, ca = m2.generate_continued("Hello there.", VOICE)
    pcm_b, cb = m2.generate_continued("General greeting.", VOICE, ca)
    assert ca.slot == 0 and ca.latents.shape == (pcm_a.shape[1] // 1920, 32)
    assert eng2.admit_log[1][1] == ca.ids.tolist() + cb.ids.tolist() and eng2.admit_log[1][3]
    np.testing.assert_array_equal(eng2.admit_log[1][2], ca.latents)
    assert pcm_b.shape[1] // 1920 == cb.latents.shape[0]  # only the new frames
