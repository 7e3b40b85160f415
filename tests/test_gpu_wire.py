"""Wire-format output from the device (ptts_wire_enable / ptts_slots_open_opts / ptts_fetch_wire):
rows with different sample rates and encodings, and rows with none, share one batch; a wire row's
chunks, concatenated, are byte for byte the numpy encoding rule applied to Engine.resample (the
whole-signal kernel the voice front-end tests pin) of the row's own concatenated f32 frames; the
chunk sizes are the table of include/pocket_tts.h; and nothing else the engine returns changes.

Independent of the project's resampler, a float64 numpy restatement of scipy's resample_poly
(firwin with a Kaiser(5) window, polyphase upfirdn) written here gives every 16-bit sample within 1
and every G.711 code within one code step: float rounding can straddle a truncation boundary,
never more.

Small engines: 4 slots, synthetic weights, temp 0, EOS off, 1 to 9 frames per row with different
lengths per row, so `last` falls at different places in a pass."""

from math import gcd

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INF = float("inf")
MODES = [(False, 1), (True, 1), (True, 2), (True, 4)]  # (pipeline, back_frames)
BYTES = {"pcm_s16le": 2, "ulaw": 1, "alaw": 1}
# per-frame chunk sizes in samples: (first, middle, last)
CHUNKS = {8000: (630, 640, 650), 16000: (1270, 1280, 1290), 24000: (1920, 1920, 1920),
          44100: (3510, 3528, 3546), 48000: (3820, 3840, 3860)}
CASE_A = [None, (24000, "pcm_s16le"), (8000, "ulaw"), (48000, "pcm_s16le")]
CASE_B = [(16000, "alaw"), None, (44100, "pcm_s16le"), (8000, "alaw")]
# s -> (mu-law, A-law): the pinned values of the issue
PINNED = {0: (0xFF, 0xD5), -1: (0x7E, 0x55), 4: (0xFE, 0xD5), 100: (0xF2, 0xD3), 1000: (0xCE, 0xFA),
          -1000: (0x4E, 0x7A), 32767: (0x80, 0xAA), -32768: (0x00, 0x2A)}


# ---------------------------------------------------------------- the numpy side
def np_s16(x):
    """trunc(clamp(x, -1, 1) * 32767) in float32"""
    return (np.clip(np.asarray(x, np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)


def np_ulaw(s):
    out = np.zeros(len(s), np.uint8)
    ends = [0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF]
    for i, x in enumerate(np.asarray(s, np.int64).tolist()):
        v = x >> 2
        mask = 0x7F if v < 0 else 0xFF
        v = min(abs(v), 8159) + 33
        seg = next((k for k, e in enumerate(ends) if v <= e), 8)
        out[i] = (0x7F ^ mask) if seg == 8 else (((seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask)
    return out


def np_alaw(s):
    out = np.zeros(len(s), np.uint8)
    ends = [0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF]
    for i, x in enumerate(np.asarray(s, np.int64).tolist()):
        v, mask = (x >> 3, 0xD5) if x >= 0 else ((-x - 1) >> 3, 0x55)
        seg = next(k for k, e in enumerate(ends) if v <= e)
        out[i] = ((seg << 4) | ((v >> (1 if seg < 2 else seg)) & 15)) ^ mask
    return out


_LUT = {}


def g711(s, enc):
    """codes of 16-bit values, through a table of the scalar rule above"""
    if enc not in _LUT:
        _LUT[enc] = (np_ulaw if enc == "ulaw" else np_alaw)(np.arange(-32768, 32768))
    return _LUT[enc][np.asarray(s, np.int32) + 32768]


def np_encode(x, enc):
    """float32 samples at the wire rate -> bytes"""
    s = np_s16(x)
    return s.astype("<i2").tobytes() if enc == "pcm_s16le" else g711(s, enc).tobytes()


def code_index(codes, enc):
    """G.711 codes on a monotone integer scale (adjacent quantizer cells differ by 1)"""
    c = np.asarray(codes, np.uint8).astype(np.int32)
    if enc == "ulaw":
        mag = (~c) & 0x7F
        return np.where(c & 0x80, mag, -mag)  # a negative cell 0 does not exist
    c = c ^ 0x55
    mag = c & 0x7F
    return np.where(c & 0x80, mag, -mag - 1)


def resample_poly_f64(x, rate):
    """scipy.signal.resample_poly(x, up, down) from 24 kHz in float64: firwin(2 half + 1, 1 / max
    rate, window=("kaiser", 5.0)) * up, zero-stuffed convolution, every down-th sample from `half`."""
    g = gcd(24000, rate)
    up, down = rate // g, 24000 // g
    mr = max(up, down)
    half = 10 * mr
    L = 2 * half + 1
    k = np.arange(L, dtype=np.float64) - half
    win = np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (k / half) ** 2))) / np.i0(5.0)
    h = np.sinc(k / mr) / mr * win
    h = h / h.sum() * up
    x = np.asarray(x, np.float64)
    n = len(x)
    n_out = -(-n * up // down)
    a = np.arange(n_out, dtype=np.int64) * down + half  # tap index of x[0]
    K = L // up + 2
    j = (a // up)[:, None] - np.arange(K, dtype=np.int64)[None, :]
    idx = a[:, None] - j * up
    ok = (j >= 0) & (j < n) & (idx >= 0) & (idx < L)
    return (np.where(ok, x[np.clip(j, 0, n - 1)], 0.0) * np.where(ok, h[np.clip(idx, 0, L - 1)], 0.0)).sum(axis=1)


def expected_chunks(rate, enc, n_frames):
    if n_frames == 1:
        sizes = [1920 * rate // 24000]
    else:
        first, mid, last = CHUNKS[rate]
        sizes = [first] + [mid] * (n_frames - 2) + [last]
    return [s * BYTES[enc] for s in sizes]


# ---------------------------------------------------------------- the engine side
def params(max_frames, fmt=None):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1)
    if fmt:
        p.sample_rate, p.encoding = fmt
    return p


def engine(mode, wire=True, slots=4):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=slots, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=mode[0],
                     back_frames=mode[1], wire=wire)


def admit(eng, formats, frames, voice, slots=None):
    slots = list(range(len(formats))) if slots is None else slots
    rng = np.random.default_rng(5)
    ids = [rng.integers(0, 4000, size=3 + b).astype(np.int32) for b in slots]
    eng.open_many(slots, [voice] * len(slots), ids, [params(frames[i], formats[i]) for i in range(len(slots))])


def make_voice(eng):
    prompt = (0.11 * np.random.default_rng(3).standard_normal((4, 1024))).astype(np.float32)
    return eng.voice_from_prompt(prompt)


def drive(eng, B, frames, rows_for_call=None, record=None):
    """Step until every row's last frame is fetched (flush calls once no row has a frame left to
    start). Per row: its f32 frames, its wire chunks (non-empty ones), and the bytes returned for
    frames the row did not have. record: a list that receives every call's raw outputs."""
    started = [0] * B
    got = [0] * B
    pcm = [[] for _ in range(B)]
    wire = [[] for _ in range(B)]
    call, delay = 0, eng.frame_lag()[1]
    while any(got[b] < frames[b] for b in range(B)):
        assert call < 64, "the rows never finished"
        if all(started[b] >= frames[b] for b in range(B)) and eng.pipeline:
            eng.flush_async(B)
            n = B
        else:
            n = rows_for_call(call) if rows_for_call else B
            eng.step_async(n)
            for b in range(n if call >= delay else 0):  # rows admitted inside a pass start at the next
                started[b] += started[b] < frames[b]
        r = eng.fetch(B)  # all rows: a paused row's earlier frames still arrive
        w = eng.fetch_wire(B) if eng.wire else [b""] * B
        if record is not None:
            record.append((r.pcm.copy(), r.valid.copy(), r.last.copy(), r.eos_logits.copy(), r.latents.copy()))
        for b in range(B):
            if r.valid[b]:
                got[b] += 1
                pcm[b].append(r.pcm[b].copy())
                wire[b].append(w[b])
                assert bool(r.last[b]) == (got[b] == frames[b]), (b, got[b])
            else:
                assert w[b] == b"", (call, b, len(w[b]))
        call += 1
    return pcm, wire


def check_rows(eng, formats, frames, pcm, wire, tag=""):
    """every wire row against Engine.resample + the numpy rule (exact) and against the float64
    restatement (within one step); rows with no format returned no bytes"""
    for b, fmt in enumerate(formats):
        assert len(pcm[b]) == frames[b]
        if fmt is None:
            assert all(c == b"" for c in wire[b]), (tag, b)
            continue
        rate, enc = fmt
        x = np.concatenate(pcm[b])
        assert [len(c) for c in wire[b]] == expected_chunks(rate, enc, frames[b]), (tag, b, fmt)
        y = x if rate == 24000 else eng.resample(x, 24000, rate)
        got = b"".join(wire[b])
        want = np_encode(y, enc)
        assert len(got) == len(want), (tag, b, fmt, len(got), len(want))
        if got != want:
            g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{tag} row {b} {fmt}: {bad.size} bytes differ, first at {bad[0]}")
        # the independent float64 reference
        s64 = np.trunc(np.clip(resample_poly_f64(x, rate), -1.0, 1.0) * 32767.0).astype(np.int32)
        if enc == "pcm_s16le":
            worst = int(np.abs(np.frombuffer(got, "<i2").astype(np.int32) - s64).max())
        else:
            worst = int(np.abs(code_index(np.frombuffer(got, np.uint8), enc) - code_index(g711(s64, enc), enc)).max())
        print(f"{tag} row {b} {fmt}: {len(got)} bytes exact; worst step vs float64 {worst}")
        assert worst <= 1, (tag, b, fmt, worst)


@pytest.mark.parametrize("pipeline,back_frames", MODES)
def test_mixed_formats_share_a_batch(pipeline, back_frames):
    """Case A then case B on one engine (the slots are re-admitted with other formats): rows of
    3 to 9 frames, every wire row exact, chunk sizes by the table, no bytes for rows with none."""
    eng = engine((pipeline, back_frames))
    try:
        v = make_voice(eng)
        for tag, formats, frames in (("A", CASE_A, [5, 9, 3, 6]), ("B", CASE_B, [4, 3, 7, 5])):
            admit(eng, formats, frames, v)
            pcm, wire = drive(eng, 4, frames)
            check_rows(eng, formats, frames, pcm, wire, f"{tag} pipeline={pipeline} bf={back_frames}")
    finally:
        eng.close()


@pytest.mark.parametrize("pipeline,back_frames", [(False, 1), (True, 2)])
def test_wire_changes_nothing_else(pipeline, back_frames):
    """The same batch on an engine without wire output: PCM, latents, EOS logits and flags of every
    call are exactly the wire-enabled run's."""
    frames = [5, 9, 3, 6]
    out = []
    for wire in (True, False):
        eng = engine((pipeline, back_frames), wire=wire)
        try:
            admit(eng, CASE_A if wire else [None] * 4, frames, make_voice(eng))
            rec = []
            drive(eng, 4, frames, record=rec)
            out.append(rec)
        finally:
            eng.close()
    assert len(out[0]) == len(out[1])
    for a, b in zip(out[0], out[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("pipeline,back_frames", [(False, 1), (True, 4)])
def test_one_frame_utterances_and_paused_rows(pipeline, back_frames):
    """Rows 0 and 1 are one-frame utterances (a single chunk of 1920 up / down samples); calls 4-7
    cover three rows only, so row 3 pauses inside its utterance: it emits nothing then and loses
    nothing; the partial last pass is drained by flush calls."""
    formats = [(8000, "ulaw"), (44100, "pcm_s16le"), (16000, "pcm_s16le"), (48000, "alaw")]
    frames = [1, 1, 7, 9]
    eng = engine((pipeline, back_frames))
    try:
        admit(eng, formats, frames, make_voice(eng))
        pcm, wire = drive(eng, 4, frames, rows_for_call=lambda k: 3 if 4 <= k < 8 else 4)
        assert len(wire[0][0]) == 640 and len(wire[1][0]) == 3528 * 2
        check_rows(eng, formats, frames, pcm, wire, f"edges pipeline={pipeline} bf={back_frames}")
    finally:
        eng.close()


@pytest.mark.parametrize("back_frames", [1, 2])
def test_slot_readmitted_before_its_last_frame_is_fetched(back_frames):
    """A driver that keeps one call in flight (call k + 1 is issued, then call k is fetched): slot 0
    runs a 4-frame 8 kHz mu-law utterance and is re-admitted as 48 kHz 16-bit while the pass that
    decodes its last frame is in flight and unfetched. The new row's bytes equal a fresh engine's (no
    tail of the old row leaks) and the old row's last chunks still arrive intact."""
    new_fmt, new_frames, old_frames = (48000, "pcm_s16le"), 4, 4
    fresh = engine((True, back_frames), slots=1)
    try:
        admit(fresh, [new_fmt], [new_frames], make_voice(fresh))
        _, want = drive(fresh, 1, [new_frames])
    finally:
        fresh.close()
    eng = engine((True, back_frames), slots=1)
    try:
        v = make_voice(eng)
        admit(eng, [(8000, "ulaw")], [old_frames], v)
        old_pcm, old_wire, new_wire = [], [], []

        def take():  # the frame of the call before the latest
            r, w = eng.fetch(1, calls_back=1), eng.fetch_wire(1, calls_back=1)
            if not r.valid[0]:
                assert w[0] == b""
            elif len(old_pcm) < old_frames:
                old_pcm.append(r.pcm[0].copy())
                old_wire.append(w[0])
            else:
                new_wire.append(w[0])

        for k in range(old_frames + 1):  # call old_frames launches the pass over the last frame
            eng.step_async(1)
            if k:
                take()
        assert len(old_pcm) < old_frames  # the last frame is not fetched yet
        admit(eng, [new_fmt], [new_frames], v)
        for _ in range(32):
            if len(new_wire) == new_frames:
                break
            eng.step_async(1)
            take()
        assert len(old_pcm) == old_frames
        assert new_wire == want[0]
        check_rows(eng, [(8000, "ulaw")], [old_frames], [old_pcm], [old_wire], "old row")
    finally:
        eng.close()


def test_encode_wire_all_values_and_resample_path():
    """The seam alone: inputs (k + 0.5 sign(k)) / 32767 for all 65,536 k; every encoding equals the
    numpy rule and the pinned table; at 8 kHz it equals resample + encode."""
    eng = engine((False, 1), wire=False, slots=1)
    try:
        k = np.arange(-32768, 32768)
        x = ((k + 0.5 * np.sign(k)) / 32767.0).astype(np.float32)
        s = np_s16(x)
        assert np.array_equal(s[1:-1], k[1:-1]) and s[0] == -32767 and s[-1] == 32767  # the ends clamp
        for enc in ("pcm_s16le", "ulaw", "alaw"):
            assert eng.encode_wire(x, 24000, enc) == np_encode(x, enc), enc
        for sv, (u, a) in PINNED.items():
            one = np.array([sv / 32767.0 + (0.25 / 32767.0) * np.sign(sv)], np.float32)
            assert int(np_s16(one)[0]) == max(sv, -32767)
            assert np_ulaw([sv])[0] == u and np_alaw([sv])[0] == a, sv
            if sv != -32768:  # not reachable from a clamped float
                assert eng.encode_wire(one, 24000, "ulaw")[0] == u and eng.encode_wire(one, 24000, "alaw")[0] == a
        y = (0.3 * np.sin(np.arange(5000) * 0.01) + 0.1 * np.random.default_rng(0).standard_normal(5000))
        y = y.astype(np.float32)
        for enc in ("pcm_s16le", "ulaw", "alaw"):
            assert eng.encode_wire(y, 8000, enc) == np_encode(eng.resample(y, 24000, 8000), enc), enc
    finally:
        eng.close()


def test_refusals_admit_nothing():
    import pocket_tts_amd as pt

    plain = engine((False, 1), wire=False, slots=1)
    wired = engine((False, 1), wire=True, slots=1)
    try:
        for eng, fmt in ((plain, (8000, "ulaw")), (wired, (22050, "pcm_s16le")), (wired, (8000, 9))):
            with pytest.raises(pt.PocketTTSError) as e:
                admit(eng, [fmt], [2], make_voice(eng))
            assert e.value.code == 1, fmt
            r = eng.step(1)
            assert not r.valid[0], fmt  # nothing was admitted
        with pytest.raises(pt.PocketTTSError):
            plain.fetch_wire(1)
        wired.step(1)
        with pytest.raises(pt.PocketTTSError):  # after the first step
            from pocket_tts_amd._lib import check, lib

            check(lib().ptts_wire_enable(wired.handle, 0))
    finally:
        plain.close()
        wired.close()


def test_tts_model_returns_wire_bytes():
    """TTSModel.generate / generate_stream with sample_rate / encoding: bytes, equal to the numpy
    rule on Engine.resample of what generate returns without them (temp 0: the same PCM)."""
    import pocket_tts_amd as pt

    eng = engine((True, 2), slots=1)
    try:
        m = pt.TTSModel(eng, temp=0.0, lsd_decode_steps=1, eos_threshold=INF, noise_clamp=None)
        v = make_voice(eng)
        ids = np.array([260, 2994, 262, 578], np.int32)
        x = m.generate(ids, v, max_frames=4)
        assert x.dtype == np.float32 and x.shape == (1, 4 * 1920)
        got = m.generate(ids, v, max_frames=4, sample_rate=16000, encoding="ulaw")
        assert isinstance(got, bytes) and got == np_encode(eng.resample(x[0], 24000, 16000), "ulaw")
        chunks = list(m.generate_stream(ids, v, max_frames=4, encoding="pcm_s16le"))  # rate: 24 kHz
        assert [len(c) for c in chunks] == [3840] * 4 and b"".join(chunks) == np_encode(x[0], "pcm_s16le")
    finally:
        eng.close()


def test_scheduler_hands_out_the_engines_bytes():
    """The server's scheduler on a real wire-enabled engine (previews off, so every row's frame 0 is
    the regular one): four requests with the same text in one batch, one plain and three with
    formats; the wire requests' bytes are the numpy rule on Engine.resample of the plain one's PCM."""
    from pocket_tts_amd.serve import BatchScheduler

    eng = engine((True, 2))
    sch = BatchScheduler(eng, preview_rows=0)
    try:
        v = sch.call(lambda: make_voice(eng))
        formats = [None, (8000, "ulaw"), (48000, "pcm_s16le"), (24000, "alaw")]
        reqs = [sch.submit(np.array([260, 2994, 262], np.int32), v, params(5, f)) for f in formats]
        x = reqs[0].audio(timeout=60)
        assert x.shape == (5 * 1920,)
        for f, r in zip(formats[1:], reqs[1:]):
            got = r.wire_audio(timeout=60)
            y = x if f[0] == 24000 else sch.call(lambda: eng.resample(x, 24000, f[0]))
            assert got == np_encode(y, f[1]), f
    finally:
        sch.close()
        eng.close()
