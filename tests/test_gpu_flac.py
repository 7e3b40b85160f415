"""The FLAC stage on the GPU (ptts_flac_enable / PTTS_WIRE_FLAC / ptts_flac_encode; DESIGN.md section
21): the seam against the host restatement audio.flac_frames byte for byte and against the
independent decoder of tests/flac_decode.py; FLAC rows streaming beside other rows; the tempo stage
ahead of it (chunks of several frames); re-admission; and the refusals.

Small engines: at most 4 slots, synthetic weights, temp 0, EOS off."""

import numpy as np
import pytest

import flac_decode as fd
from test_flac import SIGNALS, SIZES, firsts, signal
from test_gpu_wire import CHUNKS, drive, make_voice

pytestmark = pytest.mark.gpu

INF = float("inf")
ROWS = [(24000, "flac"), (8000, "flac"), (8000, "pcm_s16le"), None]
PLAIN = [(24000, "pcm_s16le"), (8000, "pcm_s16le"), (8000, "pcm_s16le"), None]  # the same rows without FLAC


def params(max_frames, fmt=None, speed=None):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1)
    if fmt:
        p.sample_rate, p.encoding = fmt
    p.speed = speed
    return p


def engine(pipeline=False, back_frames=1, flac=True, tempo=False, slots=4):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=slots, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=pipeline,
                     back_frames=back_frames, wire=True, tempo=tempo, flac=flac)


def admit(eng, formats, frames, voice, speed=None):
    rng = np.random.default_rng(5)
    slots = list(range(len(formats)))
    ids = [rng.integers(0, 4000, size=3 + b).astype(np.int32) for b in slots]
    eng.open_many(slots, [voice] * len(slots), ids, [params(frames[i], formats[i], speed) for i in slots])


@pytest.fixture(scope="module")
def seam():
    eng = engine(slots=1)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", SIGNALS)
def test_seam_equals_the_host_rule(seam, name):
    """every size x signal (one first-sample value per size, all of them at n = 640)"""
    from pocket_tts_amd.audio import flac_frames

    for n in SIZES:
        s = signal(name, n)
        for first in (firsts(n) if n == 640 else (firsts(n)[SIZES.index(n) % 13],)):
            rate = (8000, 16000, 24000, 44100, 48000)[SIZES.index(n) % 5]
            got = seam.flac_encode(s, rate, first)
            assert got == flac_frames(s, first, rate), (name, n, first)
            dec, info = fd.decode_frames(got, rate)
            assert np.array_equal(dec, s) and info[0][0] == first
            assert all(size <= 17 + 2 * m for _, m, size in info)


def run(mode, formats, flac, frames=6):
    eng = engine(True, mode, flac=flac)
    try:
        rec = []
        admit(eng, formats, [frames] * 4, make_voice(eng))
        pcm, wire = drive(eng, 4, [frames] * 4, record=rec)
        return pcm, wire, rec
    finally:
        eng.close()


@pytest.mark.parametrize("back_frames", [1, 4])
def test_flac_rows_stream_beside_other_rows(back_frames):
    from pocket_tts_amd.audio import flac_frames

    pcm, wire, rec = run(back_frames, ROWS, True)
    pcm0, wire0, rec0 = run(back_frames, PLAIN, False)
    # nothing but the FLAC rows' bytes depends on the stage
    assert len(rec) == len(rec0)
    for a, b in zip(rec, rec0):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert wire[2] == wire0[2] and b"".join(wire[2]) != b"" and all(c == b"" for c in wire[3])
    eng = engine(slots=1)
    try:
        for b, (rate, _) in enumerate(ROWS[:2]):
            want = eng.encode_wire(np.concatenate(pcm[b]), rate, "pcm_s16le")
            assert want == b"".join(wire0[b])
            at, sizes = 0, []
            for chunk in wire[b]:
                s, info = fd.decode_frames(chunk, rate)
                assert len(info) == 1 and info[0][0] == at, (b, info, at)  # contiguous from 0, one frame per chunk
                assert chunk == flac_frames(s, at, rate), (b, at)
                assert chunk == eng.flac_encode(s, rate, at)
                assert s.astype("<i2").tobytes() == want[2 * at:2 * (at + s.size)]
                at += s.size
                sizes.append(s.size)
            assert 2 * at == len(want)
            first, mid, last = CHUNKS[rate]
            assert sizes == [first] + [mid] * 4 + [last], (b, sizes)
            print(f"back_frames {back_frames} row {b} at {rate} Hz: {sum(map(len, wire[b]))} FLAC bytes for "
                  f"{len(want)} of s16: {sum(map(len, wire[b])) / len(want):.3f}")
    finally:
        eng.close()


def test_tempo_chunks_hold_several_frames():
    eng = engine(True, 1, tempo=True, slots=1)
    try:
        admit(eng, [(48000, "flac")], [3], make_voice(eng), speed=0.5)
        pcm, wire = drive(eng, 1, [3])
        want = eng.encode_wire(eng.tempo(np.concatenate(pcm[0]), 0.5), 48000, "pcm_s16le")
        at, got = 0, []
        for chunk in wire[0]:
            if not chunk:
                continue
            s, info = fd.decode_frames(chunk, 48000)
            assert info[0][0] == at and [n for _, n, _ in info[:-1]] == [4608] * (len(info) - 1)
            at += s.size
            got.append((s, len(info)))
        assert got[-1][0].size > 4608 and got[-1][1] in (2, 3)
        assert np.concatenate([s for s, _ in got]).astype("<i2").tobytes() == want
    finally:
        eng.close()


def test_readmission_restarts_the_sample_numbers():
    eng = engine(True, 4, slots=2)
    try:
        voice = make_voice(eng)
        for frames in (3, 2):
            admit(eng, [(16000, "flac")], [frames], voice)
            _, wire = drive(eng, 1, [frames])
            data = b"".join(wire[0])
            s, info = fd.decode_frames(data, 16000)
            assert info[0][0] == 0 and s.size == frames * 1280
            assert [a for a, _, _ in info] == list(np.cumsum([0] + [n for _, n, _ in info[:-1]]))
    finally:
        eng.close()


def test_refusals():
    import pocket_tts_amd as pt
    from pocket_tts_amd._lib import check, lib

    plain = engine(flac=False, slots=1)
    on = engine(slots=1)
    try:
        with pytest.raises(pt.PocketTTSError) as e:
            admit(plain, [(24000, "flac")], [2], make_voice(plain))
        assert e.value.code == 1
        for _ in range(3):
            plain.step_async(1)
            assert not plain.fetch(1).valid[0]  # nothing was admitted
        with pytest.raises(pt.PocketTTSError) as e:
            plain.encode_wire(np.zeros(1920, np.float32), 24000, "flac")
        admit(on, [(24000, "flac")], [2], make_voice(on))
        on.step_async(1)
        with pytest.raises(pt.PocketTTSError) as e:  # after the first step
            check(lib().ptts_flac_enable(on.handle, 0))
        assert e.value.code == 1
        with pytest.raises(pt.PocketTTSError):  # not wire-enabled
            pt.Engine(device=0, max_slots=1, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, flac=True)
    finally:
        plain.close()
        on.close()
