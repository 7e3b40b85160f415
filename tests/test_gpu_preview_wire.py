"""First-frame previews on an engine that also runs the wire and tempo stages: the configuration the
server runs (serve.py), which the preview tests (no wire stage) and the wire tests (no previews) each
cover half of.

A preview pass decodes to f32 only: it must neither run the wire / tempo ops nor touch their per-row
state, so with previews on, every row's f32 frames and wire bytes are exactly those of the same
schedule without previews, and each preview is its row's regular frame 0 up to the float rounding of
the other tile shapes (the bound of test_gpu_preview). decode_latents is the other pass that leaves
the wire stage out: a row admitted after it gets the bytes a fresh engine gives.

Small engines: 4 slots, synthetic weights, temp 0, EOS off, two-frame passes; three rows admitted in
one call (none / a format / a format and a speed) and one admitted inside a pass."""

import numpy as np
import pytest
from conftest import PCM_TOL, pcm_err

pytestmark = pytest.mark.gpu

INF = float("inf")
S = 4
# slot -> (frames, (sample_rate, encoding) or None, speed or None)
ROWS = {0: (10, None, None), 1: (10, (8000, "ulaw"), None), 2: (9, (16000, "pcm_s16le"), 1.25),
        3: (8, (48000, "pcm_s16le"), None)}


def params(max_frames, fmt=None, speed=None):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1, speed=speed)
    if fmt:
        p.sample_rate, p.encoding = fmt
    return p


def engine():
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=S, max_ctx=256, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                     back_frames=2, wire=True, tempo=True)


def admit(eng, voice, slots):
    rng = np.random.default_rng(11)
    ids = {b: rng.integers(0, 4000, size=3 + 2 * b).astype(np.int32) for b in sorted(ROWS)}
    eng.open_many(slots, [voice] * len(slots), [ids[b] for b in slots], [params(*ROWS[b]) for b in slots])


def make_voice(eng):
    prompt = (0.11 * np.random.default_rng(3).standard_normal((5, 1024))).astype(np.float32)
    return eng.voice_from_prompt(prompt)


def run_schedule(eng, preview_rows):
    """Rows 0-2 admitted ahead of call 0, row 3 ahead of call 1 (inside the first pass: it starts at
    call 2). Per row: its f32 frames and its wire chunks, in order; and every preview returned."""
    if preview_rows:
        eng.enable_preview(preview_rows)
    v = make_voice(eng)
    pcm = {b: [] for b in ROWS}
    wire = {b: [] for b in ROWS}
    previews = []
    admit(eng, v, [0, 1, 2])
    call = 0
    while any(len(pcm[b]) < ROWS[b][0] for b in ROWS):
        assert call < 40, "the rows never finished"
        if call == 1:
            admit(eng, v, [3])
        eng.step_async(S)
        r = eng.fetch(S)
        w = eng.fetch_wire(S)
        if preview_rows:
            previews.extend(eng.fetch_previews())
        for b in ROWS:
            if r.valid[b]:
                pcm[b].append(r.pcm[b].copy())
                wire[b].append(w[b])
                assert bool(r.last[b]) == (len(pcm[b]) == ROWS[b][0]), (b, len(pcm[b]))
            else:
                assert w[b] == b"", (call, b)
        call += 1
    if preview_rows:
        previews.extend(eng.fetch_previews(wait=True))
    return pcm, wire, previews


def test_previews_leave_pcm_and_wire_bytes_unchanged():
    out = []
    for preview_rows in (2, 0):
        eng = engine()
        try:
            out.append(run_schedule(eng, preview_rows))
        finally:
            eng.close()
    (pcm_a, wire_a, previews), (pcm_b, wire_b, none) = out
    assert none == []
    for b, (frames, fmt, _) in ROWS.items():
        assert len(pcm_a[b]) == len(pcm_b[b]) == frames, b
        for f in range(frames):
            assert np.array_equal(pcm_a[b][f], pcm_b[b][f]), (b, f)
            assert wire_a[b][f] == wire_b[b][f], (b, f)
        if fmt is None:
            assert all(c == b"" for c in wire_a[b]), b
        else:
            assert sum(len(c) for c in wire_a[b]) > 0, b
    # two previews per call: rows 0 and 1 of the first admission, then row 3 at its own start
    assert sorted(s for s, _ in previews) == [0, 1, 3]
    for slot, x in previews:
        err = pcm_err(x - pcm_a[slot][0])
        print(f"preview of row {slot}: error vs its regular frame 0 {err:.3g} (bound {PCM_TOL:.3g})")
        assert err <= PCM_TOL, slot


def test_row_admitted_after_decode_latents_gets_a_fresh_engines_bytes():
    frames, fmt, speed = 4, (16000, "pcm_s16le"), 1.25
    ids = np.array([260, 2994, 262, 578], np.int32)
    lat = (0.5 * np.random.default_rng(7).standard_normal((2, 32))).astype(np.float32)
    got = []
    for decode_first in (True, False):
        eng = engine()
        try:
            v = make_voice(eng)
            if decode_first:
                d = eng.decode_latents(0, lat)
                assert np.isfinite(d["pcm"]).all() and np.abs(d["pcm"]).max() > 0
            eng.open_many([0], [v], [ids], [params(frames, fmt, speed)])
            pcm, wire = [], []
            for call in range(40):
                if len(pcm) == frames:
                    break
                eng.step_async(1)
                r, w = eng.fetch(1), eng.fetch_wire(1)
                if r.valid[0]:
                    pcm.append(r.pcm[0].copy())
                    wire.append(w[0])
            assert len(pcm) == frames
            got.append((pcm, wire))
        finally:
            eng.close()
    assert sum(len(c) for c in got[0][1]) > 0
    assert got[0][1] == got[1][1]
    for a, b in zip(got[0][0], got[1][0]):
        assert np.array_equal(a, b)
