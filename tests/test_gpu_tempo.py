"""Per-request speech speed (ptts_tempo_enable / ptts_slot_opts.speed_permille):
the GPU tempo stage against its host restatement audio.tempo_wsola, bit for bit. The whole-signal
seam first (Engine.tempo), then rows with different speeds, rates and encodings, and rows with
none, in one batch: a speed row's chunks, concatenated, are the host pipeline over the row's own
f32 frames (tempo_wsola, then Engine.resample and the numpy encoder of test_gpu_wire.py), each
frame's byte count is the chunk-size function, and everything else equals an engine without the
stage.

Small engines: 8 slots, synthetic weights, temp 0, EOS off, 12 frames a row and one row of one."""

import numpy as np
import pytest

from test_gpu_wire import BYTES, INF, drive, expected_chunks, make_voice, np_encode

pytestmark = pytest.mark.gpu

SEAM_SPEEDS = [500, 730, 1250, 2000]
# (sample_rate, encoding, speed permille) per row; None: no format
ROWS = [None, (24000, "pcm_s16le", None), (24000, "pcm_s16le", 1000), (48000, "pcm_s16le", 500),
        (24000, "pcm_s16le", 800), (8000, "ulaw", 1250), (16000, "alaw", 2000), (48000, "pcm_s16le", 500)]
FRAMES = [12, 12, 12, 12, 12, 12, 12, 1]


def signal(n, seed=0):
    """a chirp plus seeded noise, |x| <= 0.5"""
    t = np.arange(n) / 24000.0
    x = 0.35 * np.sin(2 * np.pi * (120.0 * t + 900.0 * t * t)) + 0.03 * np.random.default_rng(seed).standard_normal(n)
    return np.clip(x, -0.5, 0.5).astype(np.float32)


def params(max_frames, row):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1)
    if row:
        p.sample_rate, p.encoding = row[0], row[1]
        p.speed = None if row[2] is None else row[2] / 1000.0
    return p


def engine(back_frames, tempo=True, slots=8, wire=True):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=slots, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                     back_frames=back_frames, wire=wire, tempo=tempo)


def admit(eng, rows, frames, voice, slots=None):
    slots = list(range(len(rows))) if slots is None else slots
    rng = np.random.default_rng(5)
    ids = [rng.integers(0, 4000, size=3 + b).astype(np.int32) for b in slots]
    eng.open_many(slots, [voice] * len(slots), ids, [params(frames[i], rows[i]) for i in range(len(slots))])


def host_pipeline(eng, pcm_frames, row):
    """(all bytes, per-frame byte counts) of a speed row by the host rule over its f32 frames"""
    from pocket_tts_amd.audio import tempo_chunk_samples, tempo_wsola

    rate, enc, sp = row
    n = len(pcm_frames)
    y = tempo_wsola(np.concatenate(pcm_frames), sp)
    z = y if rate == 24000 else eng.resample(y, 24000, rate)
    # the resampler's streaming rule over the tempo chunks: emitted(N) outputs after N inputs
    g = np.gcd(24000, rate)
    up, down = rate // g, 24000 // g
    half = 10 * max(up, down)
    sizes, seen, out = [], 0, 0
    for f in range(n):
        seen += tempo_chunk_samples(f, sp, f == n - 1)
        if f == n - 1:
            m = -(-seen * up // down)
        else:
            m = seen if rate == 24000 else (0 if seen == 0 else (seen * up - 1 - half) // down + 1)
        sizes.append((m - out) * BYTES[enc])
        out = m
    assert seen == len(y)
    return np_encode(z, enc), sizes


@pytest.fixture(scope="module")
def seam_engine():
    eng = engine(1, tempo=False, slots=1, wire=False)
    yield eng
    eng.close()


@pytest.mark.parametrize("sp", SEAM_SPEEDS)
def test_seam_equals_the_host_rule(seam_engine, sp):
    from pocket_tts_amd.audio import tempo_len, tempo_wsola

    x = signal(24000)
    got = seam_engine.tempo(x, sp / 1000.0)
    want = tempo_wsola(x, sp)
    assert len(got) == tempo_len(24000, sp) == seam_engine.tempo_len(24000, sp / 1000.0)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"sp {sp}: {bad.size} samples differ, first at {bad[0]}"


@pytest.mark.parametrize("n", [1, 239, 1920])
def test_seam_short_signals(seam_engine, n):
    from pocket_tts_amd.audio import tempo_wsola

    x = signal(n, seed=n)
    for sp in SEAM_SPEEDS:
        got, want = seam_engine.tempo(x, sp / 1000.0), tempo_wsola(x, sp)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, sp)


_PLAIN = {}


def plain_run(back_frames):
    """the batch on an engine without the tempo stage (speeds dropped): the reference of every
    output that must not depend on speed, computed once per pass shape"""
    if back_frames not in _PLAIN:
        eng = engine(back_frames, tempo=False)
        try:
            rows = [r and (r[0], r[1], None) for r in ROWS]
            admit(eng, rows, FRAMES, make_voice(eng))
            rec = []
            pcm, wire = drive(eng, 8, FRAMES, record=rec)
            _PLAIN[back_frames] = (pcm, wire, rec)
        finally:
            eng.close()
    return _PLAIN[back_frames]


@pytest.mark.parametrize("back_frames", [1, 4])
def test_speed_rows_in_a_mixed_batch(back_frames):
    eng = engine(back_frames)
    try:
        admit(eng, ROWS, FRAMES, make_voice(eng))
        rec = []
        pcm, wire = drive(eng, 8, FRAMES, record=rec)
        ppcm, pwire, prec = plain_run(back_frames)
        # f32 PCM, flags, EOS logits and latents of every call: those of the engine without the stage
        assert len(rec) == len(prec)
        for a, b in zip(rec, prec):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        for b, row in enumerate(ROWS):
            assert len(pcm[b]) == FRAMES[b]
            if row is None or row[2] in (None, 1000):  # no speed: today's bytes
                assert wire[b] == pwire[b], b
                if row:
                    assert [len(c) for c in wire[b]] == expected_chunks(row[0], row[1], FRAMES[b])
                continue
            want, sizes = host_pipeline(eng, pcm[b], row)
            got = b"".join(wire[b])
            print(f"bf={back_frames} row {b} {row}: {len(got)} bytes, chunks {[len(c) for c in wire[b]]}")
            assert [len(c) for c in wire[b]] == sizes, (b, row)
            assert len(got) == len(want), (b, row, len(got), len(want))
            if got != want:
                g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
                bad = np.flatnonzero(g != w)
                raise AssertionError(f"row {b} {row}: {bad.size} bytes differ, first at {bad[0]}")
    finally:
        eng.close()


def test_slot_readmitted_with_another_speed_and_cancel():
    """One call in flight (call k + 1 issued, then call k fetched): slot 0 runs a 4-frame row at
    speed 2000 and is re-admitted at speed 500, 48 kHz, while the pass over its last frame is
    unfetched; the new row's bytes equal a fresh engine's. Then the row is cancelled mid-utterance:
    no byte of it arrives afterwards."""
    old, new, nf = (8000, "ulaw", 2000), (48000, "pcm_s16le", 500), 4
    fresh = engine(2, slots=1)
    try:
        admit(fresh, [new], [nf], make_voice(fresh))
        _, want = drive(fresh, 1, [nf])
    finally:
        fresh.close()
    eng = engine(2, slots=1)
    try:
        v = make_voice(eng)
        admit(eng, [old], [nf], v)
        old_pcm, old_wire, new_wire = [], [], []

        def take():
            r, w = eng.fetch(1, calls_back=1), eng.fetch_wire(1, calls_back=1)
            if not r.valid[0]:
                assert w[0] == b""
            elif len(old_pcm) < nf:
                old_pcm.append(r.pcm[0].copy())
                old_wire.append(w[0])
            else:
                new_wire.append(w[0])

        for k in range(nf + 1):
            eng.step_async(1)
            if k:
                take()
        assert len(old_pcm) < nf
        admit(eng, [new], [nf], v)
        for _ in range(32):
            if len(new_wire) == nf:
                break
            eng.step_async(1)
            take()
        assert len(old_pcm) == nf
        assert new_wire == want[0]
        assert b"".join(old_wire) == host_pipeline(eng, old_pcm, old)[0]
        # cancel: a 12-frame speed row, cancelled after a few calls
        admit(eng, [new], [12], v)
        for _ in range(5):
            eng.step_async(1)
        eng.cancel_slots([0])
        for _ in range(10):
            eng.step_async(1)
            assert eng.fetch_wire(1) == [b""] and not eng.fetch(1).valid[0]
    finally:
        eng.close()


def test_refusals_admit_nothing():
    import ctypes as C

    import pocket_tts_amd as pt
    from pocket_tts_amd._lib import WIRE_CHUNK_MAX, WIRE_CHUNK_MAX_TEMPO, check, lib, u8ptr

    wired = engine(1, tempo=False, slots=1)
    tempo = engine(1, slots=1)
    try:
        for eng, sp in ((tempo, 0.499), (tempo, 2.001), (wired, 0.8)):
            with pytest.raises(pt.PocketTTSError) as e:
                admit(eng, [(24000, "pcm_s16le", sp * 1000)], [2], make_voice(eng))
            assert e.value.code == 1, sp
            for _ in range(3):
                eng.step_async(1)
                assert not eng.fetch(1).valid[0], sp  # nothing was admitted
        buf = np.zeros(WIRE_CHUNK_MAX_TEMPO, np.uint8)
        n = np.zeros(1, np.int32)
        with pytest.raises(pt.PocketTTSError) as e:  # the stride of an engine without the stage
            check(lib().ptts_fetch_wire(tempo.handle, 0, 1, u8ptr(buf), WIRE_CHUNK_MAX,
                                        n.ctypes.data_as(C.POINTER(C.c_int))))
        assert e.value.code == 1
        check(lib().ptts_fetch_wire(tempo.handle, 0, 1, u8ptr(buf), WIRE_CHUNK_MAX_TEMPO,
                                    n.ctypes.data_as(C.POINTER(C.c_int))))
        with pytest.raises(pt.PocketTTSError):  # after the first step
            check(lib().ptts_tempo_enable(tempo.handle, 0))
        with pytest.raises(pt.PocketTTSError):  # not wire-enabled
            engine(1, slots=1, wire=False)
    finally:
        wired.close()
        tempo.close()
