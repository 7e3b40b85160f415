"""Long-form requests on the CPU: a text split into pause and sentence
segments that run as parallel rows behind one Request-like object (RequestGroup), delivered in
text order; Request.cancel() on plain requests and groups; the /stream disconnect. Driven by the
fake engine of test_serve.py (+ cancel_slots, + wire chunks) and by StandInEngine through the app.
The real-engine runs are tests/test_gpu_longform.py and tests/test_gpu_cancel.py."""

import asyncio
import json

import numpy as np
import pytest
from test_serve import VOICE, FakeEngine, params
from test_text_frontend import synthetic_tokenizer

from pocket_tts_amd.audio import pcm_i16_le_bytes, wire_bytes
from pocket_tts_amd.serve import (BatchScheduler, Request, RequestGroup, StandInEngine, TTSService, create_app,
                                  stand_in_sample)
from pocket_tts_amd.text import (estimate_frames_after_eos, long_text_segments, max_gen_len, prepare_text_prompt,
                                 silence_samples, split_into_best_sentences)

TEXT = "One, two... three. Four [pause:250ms] five"
LONG = 9000  # frames of a segment that runs until it is cancelled (the fake's max_ctx is 10,000)


class Refused(Exception):
    code = 1  # PTTS_ERR_INVALID: the admission's own requests fail, the scheduler goes on


class WireFake(FakeEngine):
    """The fake engine with wire chunks (Engine.fetch_wire: 7 bytes of value u per frame of
    utterance u), an admission that refuses utterance `refuse`, and a hook run at every step."""

    def __init__(self, max_slots=4, pipeline=False, refuse=None):
        super().__init__(max_slots=max_slots, pipeline=pipeline)
        self.wire, self.refuse, self.on_step = True, refuse, None

    def open_many(self, slots, voices, ids_list, params_list):
        if any(int(ids[0]) == self.refuse for ids in ids_list):
            raise Refused("refused utterance")
        if self.pending is not None and max(slots) >= self.pending["valid"].size:  # rows past the last call's
            grow = self.max_slots - self.pending["valid"].size
            self.pending = {k: np.concatenate([v, np.zeros((grow,) + v.shape[1:], v.dtype)])
                            for k, v in self.pending.items()}
        super().open_many(slots, voices, ids_list, params_list)

    def step_async(self, n):
        if self.on_step:
            self.on_step()
        super().step_async(n)

    def fetch_wire(self, n, calls_back=0):
        r = self.fetch(n, calls_back)
        return [bytes([int(r.pcm[s][0]) // 1000 % 256]) * 7 if r.valid[s] else b"" for s in range(n)]


class CancelFake(WireFake):
    """... and Engine.cancel_slots: the rows stop and none of their frames is reported any more."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.cancelled = []

    def cancel_slots(self, slots):
        self.cancelled.append(sorted(slots))
        held = [r for r, _ in getattr(self, "_issued", [])]
        for s in slots:
            self.rows.pop(s, None)
            if self.pending is not None and s < self.pending["valid"].size:
                self.pending["valid"][s] = False
            for r in held:
                if s < r.valid.size:
                    r.valid[s] = False


def service(eng, **kw):
    sch = BatchScheduler(eng, segment_rows=kw.pop("segment_rows", 4))
    return sch, TTSService(sch, {"v": VOICE}, default_voice="v", tokenizer=synthetic_tokenizer(), temp=0.0,
                           eos_threshold=float("inf"), **kw)


def expected_segments(text, tok):
    out = []
    for kind, val in long_text_segments(text):
        if kind == "pause":
            out.append(("pause", val))
            continue
        for c in split_into_best_sentences(val, tok.count_tokens):
            p = prepare_text_prompt(c)
            out.append(("text", list(tok(p)), max_gen_len(p), estimate_frames_after_eos(c)))
    return out


def test_segment_list():
    """The group's segments are long_text_segments with split_into_best_sentences applied, in order,
    each with its own ids, max_frames and frames_after_eos, and seeds in text order."""
    sch, svc = service(FakeEngine(max_slots=4))
    try:
        want = expected_segments(TEXT, synthetic_tokenizer())
        # ("three. Four" is one sentence chunk: short sentences share a chunk of up to 50 tokens)
        assert [w[0] for w in want] == ["text", "pause", "text", "pause", "text", "pause", "text"]
        g = svc.request(text=TEXT, long_form=True)
        assert isinstance(g, RequestGroup) and len(g.items) == len(want)
        seeds = []
        for it, w in zip(g.items, want):
            if w[0] == "pause":
                assert isinstance(it, np.ndarray) and it.shape == (silence_samples(w[1], 24000),) and not it.any()
            else:
                assert it.ids.tolist() == w[1] and it.params.max_frames == w[2] and it.params.frames_after_eos == w[3]
                seeds.append(it.params.seed)
        assert seeds == list(range(seeds[0], seeds[0] + len(seeds)))
        assert g.audio(timeout=30).size == sum(w[2] * 1920 if w[0] == "text" else silence_samples(w[1], 24000)
                                               for w in want)
    finally:
        sch.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_ordered_delivery(pipeline):
    """Segments of 5, 1, 7 and 2 frames at 3 segment rows: the stream is segment 0's frames, the
    pause, segment 1's frames, ..; never more than 3 of the group's segments wait or run; a plain
    request submitted beside it finishes first."""
    eng = WireFake(max_slots=4, pipeline=pipeline)
    sch = BatchScheduler(eng, segment_rows=3)
    try:
        lens, worst = [5, 1, 7, 2], [0]
        segs = []
        for u, n in enumerate(lens):
            segs += [("text", [u + 1, 7], params(n)), ("pause", 10 * (u + 1))]

        def probe():  # on the scheduler thread, at every step
            with sch.cv:
                held = list(sch.active.values()) + list(sch.waiting)
                worst[0] = max(worst[0], sum(r.group is not None for r in held))

        eng.on_step = probe
        with sch.cv:  # both queued before the scheduler's next pass
            g = sch.submit_group(segs, VOICE)
            plain = sch.submit([9, 7], VOICE, params(3))
        items = list(g.stream(timeout=30))
        want = []
        for u, n in enumerate(lens):
            want += [(u + 1) * 1000 + k for k in range(n)] + [("pause", silence_samples(10 * (u + 1), 24000))]
        got = [int(x[0]) if x.size == 1920 else ("pause", x.size) for x in items]
        assert got == want
        assert all(not x.any() for x in items if x.size != 1920)
        assert worst[0] == 3
        assert [int(f[0]) for f in plain.stream(timeout=30)] == [9000, 9001, 9002]
        assert plain.times["last"] < g.times["last"] and g.times["first"] <= g.times["last"]
        assert any(len(a) > 1 for a in eng.admissions)  # segments taken in one pass share an admission
        assert sch.load() == 0
    finally:
        sch.close()


@pytest.mark.parametrize("rate,enc", [(8000, "ulaw"), (24000, "pcm_s16le"), (48000, "alaw")])
def test_wire_silence(rate, enc):
    """A wire request's pauses are audio.py's encoding of silence_samples(ms, rate) zeros, in place."""
    eng = WireFake(max_slots=4, pipeline=True)
    sch, svc = service(eng)
    try:
        g = svc.request(text=TEXT, long_form=True, sample_rate=rate, encoding=enc, max_frames=3)
        assert g.wire == (rate, enc)
        items = list(g.stream(timeout=30))
        want = expected_segments(TEXT, synthetic_tokenizer())
        exp, total = [], 0
        for w in want:
            if w[0] == "pause":
                exp.append(wire_bytes(np.zeros(silence_samples(w[1], rate), np.float32), enc))
            else:
                exp += [bytes([w[1][0] % 256]) * 7] * 3  # the engine's chunks, untouched
        assert [len(x) for x in items] == [len(x) for x in exp] and items == exp
        assert all(isinstance(x, bytes) for x in items)
        pauses = [x for x, w in zip(items, exp) if len(w) != 7]
        assert pauses == [w for w in exp if len(w) != 7]
        zero = wire_bytes(np.zeros(1, np.float32), enc)
        assert all(p == zero * (len(p) // len(zero)) for p in pauses)
        total = sum(len(x) for x in exp)
        assert sum(len(x) for x in items) == total and g.out.empty()
    finally:
        sch.close()


def test_defaults_unchanged():
    """No long_form and the flag off: the plain Request of before, byte for byte; long_form with
    token_ids is refused (400); the server flag alone turns a text request into a group."""
    from fastapi.testclient import TestClient

    tok = synthetic_tokenizer()
    sch, svc = service(WireFake(max_slots=2, pipeline=True))
    try:
        r = svc.request(text="Hello world")
        assert type(r) is Request and r.group is None
        p = prepare_text_prompt("Hello world")
        assert r.ids.tolist() == list(tok(p)) and r.params.max_frames == max_gen_len(p) == 52
        assert r.params.frames_after_eos == 5 and r.params.seed == 1 and r.wire is None
        u = int(r.ids[0])
        frames = list(r.stream(timeout=30))
        assert [int(f[0]) for f in frames] == [u * 1000 + k for k in range(52)]
        c = TestClient(create_app(svc))
        got = c.post("/stream", json={"text": "Hello world"})
        assert got.status_code == 200 and got.content == pcm_i16_le_bytes(np.concatenate(frames))
        assert c.post("/generate", json={"token_ids": [3, 1], "words": 1, "long_form": True}).status_code == 400
        assert c.post("/generate", json={"token_ids": [3, 1], "words": 1, "long_form": False}).status_code == 200
        lf = c.post("/stream", json={"text": "Hello. World [pause:100ms] again", "long_form": True, "max_frames": 2})
        assert lf.status_code == 200 and len(lf.content) == 2 * (2 * 2 * 1920 + 2400)
        ov = c.post("/v1/audio/speech", json={"input": "Hello, world", "long_form": True, "response_format": "pcm"})
        assert ov.status_code == 200 and len(ov.content) == 2 * (2 * 39 * 1920 + 4800)
    finally:
        sch.close()
    sch, svc = service(FakeEngine(max_slots=2), long_form=True)
    try:
        assert isinstance(svc.request(text="Hello world"), RequestGroup)
        assert type(svc.request(token_ids=[3, 1], words=1)) is Request  # never split
        assert type(svc.request(text="Hello world", long_form=False)) is Request
    finally:
        sch.close()


def long_group(sch, first=1):
    return sch.submit_group([("text", [first + i, 7], params(LONG)) for i in range(4)], VOICE)


@pytest.mark.parametrize("kind", ["cancel_slots", "no cancel_slots"])
def test_cancel_group_midway(kind):
    """A group cancelled mid-way: the engine is told to stop exactly its active rows, its waiting
    segments are gone, load() drops, its stream ends; the next request gets the freed slot and only
    its own frames (an engine without cancel_slots: the old row's frames are told apart by step)."""
    eng = CancelFake(max_slots=4, pipeline=True) if kind == "cancel_slots" else FakeEngine(max_slots=4, pipeline=True)
    sch = BatchScheduler(eng, segment_rows=2)
    try:
        g = long_group(sch)
        it = g.stream(timeout=30)
        assert [int(next(it)[0]) for _ in range(3)] == [1000, 1001, 1002]
        assert sch.load() == 2
        g.cancel()
        sch.call(lambda: None)  # a pass of the scheduler has run since
        rest = list(it)
        assert all(int(x[0]) // 1000 == 1 for x in rest)  # what was handed over before the cancel
        assert sch.load() == 0 and not sch.waiting and not sch.active and not g.pending
        if kind == "cancel_slots":
            assert eng.cancelled == [[0, 1]]
        nxt = sch.submit([9, 7], VOICE, params(4))
        assert [int(f[0]) for f in nxt.stream(timeout=30)] == [9000, 9001, 9002, 9003]
        assert nxt.slot == 0 and sch.load() == 0
        plain = sch.submit([5, 7], VOICE, params(LONG))  # a plain request is cancelled the same way
        assert int(next(plain.stream(timeout=30))[0]) == 5000
        plain.cancel()
        sch.call(lambda: None)
        assert sch.load() == 0 and plain.ended
        if kind == "cancel_slots":
            assert eng.cancelled[-1] == [plain.slot]
        g.cancel()  # an ended request: nothing happens
        sch.call(lambda: None)
        assert sch.load() == 0
    finally:
        sch.close()


def test_stream_disconnect_cancels():
    """/stream on the StandInEngine: the client goes away after the first chunk (http.disconnect),
    the body generator is closed before the end marker and the request's rows are cancelled.
    The app is called as an ASGI application with its own receive / send: fastapi's TestClient runs
    the application to its end and buffers the body, so it cannot close a response early."""
    eng = StandInEngine(max_slots=4, max_ctx=10_000)
    sch = BatchScheduler(eng, segment_rows=2)
    svc = TTSService(sch, {"v": VOICE}, default_voice="v", tokenizer=synthetic_tokenizer())
    app = create_app(svc)
    body = json.dumps({"text": "Hello, world, again, more", "long_form": True, "max_frames": LONG}).encode()
    chunks = []

    async def run():
        sent, got = [False], asyncio.Event()

        async def receive():
            if not sent[0]:
                sent[0] = True
                return {"type": "http.request", "body": body, "more_body": False}
            await got.wait()
            return {"type": "http.disconnect"}

        async def send(msg):
            if msg["type"] == "http.response.body" and msg.get("body"):
                chunks.append(msg["body"])
                got.set()

        scope = {"type": "http", "asgi": {"version": "3.0", "spec_version": "2.3"}, "http_version": "1.1",
                 "method": "POST", "path": "/stream", "raw_path": b"/stream", "query_string": b"", "root_path": "",
                 "scheme": "http", "server": ("127.0.0.1", 8000), "client": ("127.0.0.1", 50000),
                 "headers": [(b"content-type", b"application/json"), (b"content-length", str(len(body)).encode())]}
        await app(scope, receive, send)

    try:
        asyncio.run(asyncio.wait_for(run(), 60))
        sch.call(lambda: None)
        assert chunks and len(chunks[0]) % 3840 == 0
        u = int(synthetic_tokenizer()(prepare_text_prompt("Hello"))[0])
        assert np.frombuffer(chunks[0], "<i2")[0] == int(stand_in_sample(u, 0) * 32767)
        assert sch.load() == 0 and not sch.active and not sch.waiting
        assert eng.cancelled == [[0, 1]] and not eng.rows
        nxt = sch.submit([9, 7], VOICE, params(3))
        want = [np.float32(stand_in_sample(9, k)) for k in range(3)]
        assert [f[0] for f in nxt.stream(timeout=30)] == want
    finally:
        sch.close()


def test_failing_segment_fails_the_group_once():
    """The admission of the group's third segment is refused: the consumer gets the error once and
    the end marker, the group's other rows are cancelled, and an unrelated stream is exact."""
    eng = CancelFake(max_slots=4, pipeline=True, refuse=3)
    sch = BatchScheduler(eng, segment_rows=2)
    try:
        with sch.cv:
            other = sch.submit([9, 7], VOICE, params(40))
            g = sch.submit_group([("text", [1, 7], params(4)), ("text", [2, 7], params(LONG)),
                                  ("text", [3, 7], params(5)), ("text", [4, 7], params(5))], VOICE)
        got, err = [], []
        while True:
            x = g.out.get(timeout=30)
            if x is None:
                break
            (err if isinstance(x, BaseException) else got).append(x)
        assert len(err) == 1 and isinstance(err[0], Refused)
        assert [int(x[0]) for x in got[:4]] == [1000, 1001, 1002, 1003] and all(int(x[0]) // 1000 == 2 for x in got[4:])
        assert g.out.empty()
        assert [int(f[0]) for f in other.stream(timeout=30)] == [9000 + k for k in range(40)]
        sch.call(lambda: None)
        assert sch.load() == 0 and eng.cancelled == [[2]] and not g.pending
        with pytest.raises(ValueError):  # the max_ctx rule holds per segment
            sch.submit_group([("text", [1], params(5)), ("text", [2], params(20_000))], VOICE)
        assert sch.load() == 0
    finally:
        sch.close()
