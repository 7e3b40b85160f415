"""FLAC for multi-segment responses, the server on a CPU stand-in: `long_form`
and `continuity` with FLAC answer 200 on the three audio routes and decode to exactly the samples
the same request returns as pcm_s16le; the whole-file routes state the true total; a single-segment
FLAC request keeps its bytes."""

import numpy as np
import pytest

import flac_decode as fd
from pocket_tts_amd.audio import flac_frames, flac_frames_index, flac_stream_header, pcm_i16
from pocket_tts_amd.serve import BatchScheduler, TTSService, create_app
from test_flac import VOICE, FlacFakeEngine, samples

# three text segments and two pauses; the second text piece is two sentence chunks (more than 50
# tokens together with the tokenizer below), which `continuity` chains
TEXT = "One two. [pause:200ms] Three four five six. Seven eight nine ten. [pause:15ms] Eleven."


def tokenizer(s):
    return [len(s.split())] * (7 * len(s.split()))


class IndexedFlacEngine(FlacFakeEngine):
    """The stand-in of tests/test_flac.py with the frame index beside each FLAC chunk: taken from
    audio.flac_frames_index of the same samples (which must reproduce the chunk)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.index_of = {}

    def step_async(self, n):
        super().step_async(n)
        cur = self.pending
        for s, chunk in enumerate(cur["wire"]):
            if chunk[:2] == b"\xff\xf9":
                first = fd.decode_frame(chunk, 0)[1]
                data, index = flac_frames_index(pcm_i16(cur["pcm"][s]), first, 24000)
                assert data == chunk
                self.index_of[chunk] = index

    def fetch(self, n, calls_back=0):
        r = super().fetch(n, calls_back)
        r.latents = np.zeros((r.valid.size, 32), np.float32)  # what a continuity chain keeps of its rows
        return r

    def fetch_flac_index(self, n, calls_back=0):
        return [self.index_of.get(c, []) for c in self.issued[-1 - calls_back]["wire"]][:n]


@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient

    eng = IndexedFlacEngine(max_slots=4)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"alba": VOICE}, default_voice="alba", tokenizer=tokenizer)
    try:
        yield TestClient(create_app(svc)), eng
    finally:
        sch.close()


def s16(data: bytes) -> np.ndarray:
    return np.frombuffer(data, "<i2")


def wav_data(data: bytes) -> bytes:
    at = data.index(b"data")
    return data[at + 8:]


@pytest.mark.parametrize("mode", ({"long_form": True}, {"continuity": True}, {"long_form": True, "continuity": False}))
def test_long_form_flac_is_the_pcm_of_the_same_request(client, mode):
    c, eng = client
    body = {"text": TEXT, "max_frames": 3, **mode}
    # /stream: the header with total 0, then the renumbered chunks and the pause frames in delivery order
    want = s16(c.post("/stream", json={**body, "encoding": "pcm_s16le"}).content)
    assert want.size == 4 * 3 * 1920 + 4800 + 360  # four segments of three frames, 200 ms and 15 ms at 24 kHz
    assert np.any(want[:1920]) and not np.any(want[3 * 1920:3 * 1920 + 4800])
    r = c.post("/stream", json={**body, "encoding": "flac"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
    h, got, info = fd.decode_stream(r.content)  # (asserts sample numbers contiguous from 0)
    assert (h["rate"], h["total"]) == (24000, 0) and np.array_equal(got, want)
    assert [n for _, n, _ in info] == [1920] * 3 + [4608, 192] + [1920] * 6 + [360] + [1920] * 3
    # /generate: a whole file with the true total
    want = s16(wav_data(c.post("/generate", json={**body, "encoding": "pcm_s16le"}).content))
    r = c.post("/generate", json={**body, "encoding": "flac"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
    h, got, _ = fd.decode_stream(r.content)
    assert h["total"] == want.size == 4 * 3 * 1920 + 5160 and np.array_equal(got, want)
    # /v1/audio/speech
    oa = {"input": "Hi. [pause:15ms] Yo.", **mode}  # (the route takes no max_frames: 39 frames a segment)
    want = s16(c.post("/v1/audio/speech", json={**oa, "response_format": "pcm"}).content)
    r = c.post("/v1/audio/speech", json={**oa, "response_format": "flac"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
    h, got, _ = fd.decode_stream(r.content)
    assert h["total"] == want.size == 2 * 39 * 1920 + 360 and np.array_equal(got, want)


def test_continuity_runs_its_chain_with_flac(client):
    """the chained segment is admitted behind its predecessor's latents: the rows were FLAC rows"""
    c, eng = client
    before = len(eng.admitted)
    r = c.post("/generate", json={"text": TEXT, "max_frames": 2, "continuity": True, "encoding": "flac"})
    assert r.status_code == 200
    assert eng.admitted[before:] == ["flac"] * 4
    h, got, _ = fd.decode_stream(r.content)
    assert h["total"] == got.size == 4 * 2 * 1920 + 5160


def test_a_single_segment_keeps_its_bytes(client):
    c, _ = client
    body = {"token_ids": [3, 1, 2], "max_frames": 4, "encoding": "flac"}
    frames = b"".join(flac_frames(samples(3, 4)[1920 * k:1920 * (k + 1)], 1920 * k, 24000) for k in range(4))
    assert c.post("/stream", json=body).content == flac_stream_header(24000) + frames
    assert c.post("/generate", json=body).content == flac_stream_header(24000, 4 * 1920) + frames
    r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "flac"})
    assert r.content[:42] == flac_stream_header(24000, 52 * 1920) and r.content[42:42 + len(frames)] == frames
    # one text segment of a long-form request: a group of one row, delta 0
    one = c.post("/generate", json={"text": "One two.", "max_frames": 4, "long_form": True, "encoding": "flac"})
    u = tokenizer("One two.")[0]
    frames = b"".join(flac_frames(samples(u, 4)[1920 * k:1920 * (k + 1)], 1920 * k, 24000) for k in range(4))
    assert one.status_code == 200 and one.content == flac_stream_header(24000, 4 * 1920) + frames


def test_timestamps_with_flac_stay_refused(client):
    c, eng = client
    before = len(eng.admitted)
    assert c.post("/generate", json={"text": TEXT, "long_form": True, "encoding": "flac",
                                     "timestamps": True}).status_code == 400
    assert len(eng.admitted) == before
