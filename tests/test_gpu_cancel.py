"""ptts_slots_cancel (Engine.cancel_slots): a row stops without a drain of the pipeline, the rows
beside it do not change, no fetch reports a frame of the cancelled utterance once the call has
returned, and the slot can be admitted again at once.

Every frame the engine reports is checked against the CPU oracle's run of that utterance (LAT_TOL /
PCM_TOL of conftest.py), never against another run of the engine; wire chunks are checked against
Engine.encode_wire of the row's own f32 PCM, and a re-admitted row's chunks against a fresh
engine's. Frames are attributed to utterances by the index of the call that computed them: the
fetch after call c returns frame c - frame_lag.

Small engines: 4 slots, max_ctx 256, synthetic weights, 6-frame random prompts, temp 0, EOS off."""

import numpy as np
import pytest
from conftest import LAT_TOL, PCM_TOL, pcm_err

pytestmark = pytest.mark.gpu

INF = float("inf")
MODES = [(False, 1), (True, 1), (True, 2), (True, 4)]  # (pipeline, back_frames)
FMT = {0: (8000, "ulaw"), 1: (24000, "pcm_s16le")}    # wire formats of rows 0 (kept) and 1 (cancelled)
NEW_FMT = (16000, "alaw")                              # the re-admitted row's


def utterance(i):
    """Utterance i: its own 6-frame prompt (voice) and token ids."""
    rng = np.random.default_rng(100 + i)
    prompt = (0.11 * rng.standard_normal((6, 1024))).astype(np.float32)
    return prompt, rng.integers(0, 4000, size=3 + i).astype(np.int32)


_TRAJ = {}


def oracle_frames(oracle, i, n, lsd=1, voice=None):
    """The first n frames of utterance i (voice: with another utterance's prompt) from the oracle
    (computed once per session, extended on demand)."""
    key = (i, lsd, voice)
    if key not in _TRAJ:
        prompt, ids = utterance(i if voice is None else voice)[0], utterance(i)[1]
        s = oracle.new_state(256)
        s.prefill(prompt)
        s.prefill_tokens(ids)
        _TRAJ[key] = (s, [])
    s, frames = _TRAJ[key]
    while len(frames) < n:
        o = s.step(frames[-1]["latent"] if frames else None, lsd_steps=lsd)
        frames.append({"latent": o["latent"].copy(), "pcm": o["pcm"].copy()})
    return frames[:n]


def params(max_frames, fmt=None, lsd=None):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1, lsd_steps=lsd)
    if fmt:
        p.sample_rate, p.encoding = fmt
    return p


def engine(mode, wire=True, **kw):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=4, max_ctx=256, lsd_decode_steps=1, seed=0x5EED, pipeline=mode[0],
                     back_frames=mode[1], wire=wire, **kw)


class Driver:
    """Issues calls over B rows and files every reported frame under its slot with the index of the
    call that computed it."""

    def __init__(self, eng, B):
        self.eng, self.B, self.k = eng, B, 0
        self.lag = eng.frame_lag()[0]
        self.frames = [[] for _ in range(B)]  # per slot: (fk, pcm, latent, last, wire bytes)
        self.voices = {}

    def admit(self, slots, utts, max_frames, fmts=None, lsd=None):
        for u in utts:
            if u not in self.voices:
                self.voices[u] = self.eng.voice_from_prompt(utterance(u)[0])
        self.eng.open_many(slots, [self.voices[u] for u in utts], [utterance(u)[1] for u in utts],
                           [params(max_frames, (fmts or {}).get(s), (lsd or {}).get(s)) for s in slots])
        return self.k + self.eng.frame_lag()[1]  # the call that computes the rows' first frame

    def step(self, n=1):
        for _ in range(n):
            self.eng.step_async(self.B)
            self.k += 1
            self.take(0)

    def take(self, calls_back):
        r = self.eng.fetch(self.B, calls_back=calls_back)
        w = self.eng.fetch_wire(self.B, calls_back=calls_back) if self.eng.wire else [b""] * self.B
        fk = self.k - 1 - calls_back - self.lag
        for b in range(self.B):
            if r.valid[b]:
                self.frames[b].append((fk, r.pcm[b].copy(), r.latents[b].copy(), bool(r.last[b]), w[b]))
            else:
                assert not r.last[b] and w[b] == b"", (self.k, b)
        return r, w


def check_frames(oracle, got, utt, n_total, complete, lsd=1, tag=""):
    """`got` are the first frames of utterance `utt`, oracle-exact; `last` only on frame n_total."""
    ref = oracle_frames(oracle, utt, len(got), lsd)
    for i, (fk, pcm, lat, last, _) in enumerate(got):
        e_lat, e_pcm = float(np.abs(lat - ref[i]["latent"]).max()), pcm_err(pcm - ref[i]["pcm"])
        assert e_lat <= LAT_TOL and e_pcm <= PCM_TOL, (tag, utt, i, e_lat, e_pcm)
        assert last == (i == n_total - 1), (tag, utt, i)
    if complete:
        assert len(got) == n_total, (tag, utt, len(got))


def check_wire(eng, got, fmt, tag=""):
    x = np.concatenate([f[1] for f in got])
    assert b"".join(f[4] for f in got) == eng.encode_wire(x, fmt[0], fmt[1]), (tag, fmt)


@pytest.mark.parametrize("pipeline,back_frames", MODES)
def test_cancel_mid_utterance(oracle, pipeline, back_frames):
    """Rows 1 and 2 are cancelled after 5 calls of a 12-frame batch: they report only frames of
    calls before the cancel (each oracle-exact, none last) and nothing from any fetch after it;
    rows 0 and 3 run all 12 frames, oracle-exact, row 0's wire chunks intact."""
    eng = engine((pipeline, back_frames))
    try:
        d = Driver(eng, 4)
        d.admit([0, 1, 2, 3], [0, 1, 2, 3], 12, FMT)
        d.step(5)
        before = [len(d.frames[b]) for b in range(4)]
        assert before == [max(0, 5 - d.lag)] * 4
        eng.cancel_slots([1, 2])
        for cb in (0, 1):  # from the return of the call: neither fetch reports the rows
            r, w = d.take(cb)
            assert not r.valid[1] and not r.valid[2] and w[1] == b"" and w[2] == b"", cb
        for b in (0, 3):  # (those two fetches filed frames of rows 0 and 3 a second time)
            del d.frames[b][before[b]:]
        d.step(12 + d.lag)
        tag = f"pipeline={pipeline} bf={back_frames}"
        for b in (1, 2):
            assert len(d.frames[b]) == before[b] and all(f[0] < 5 for f in d.frames[b]), (tag, b)
            check_frames(oracle, d.frames[b], b, 12, False, tag=tag)
        for b in (0, 3):
            check_frames(oracle, d.frames[b], b, 12, True, tag=tag)
        check_wire(eng, d.frames[0], FMT[0], tag)
        if d.frames[1]:
            assert all(len(f[4]) == 3840 for f in d.frames[1])  # the cancelled wire row's chunks until then
    finally:
        eng.close()


@pytest.mark.parametrize("gap", [0, 1])
@pytest.mark.parametrize("pipeline,back_frames", MODES)
def test_readmission_after_cancel(oracle, pipeline, back_frames, gap):
    """Slot 1 is cancelled and admitted again `gap` calls later with another voice, text and wire
    format: the new utterance equals its oracle from frame 0, its chunks a fresh engine's; no frame
    of the old one appears under it, and (previews on) the old one's preview is never returned."""
    fresh = engine((pipeline, back_frames))
    try:
        f = Driver(fresh, 2)
        f.admit([1], [7], 6, {1: NEW_FMT})
        f.step(6 + f.lag)
        want = [x[4] for x in f.frames[1]]
        assert len(want) == 6
    finally:
        fresh.close()
    eng = engine((pipeline, back_frames))
    try:
        if pipeline:
            eng.enable_preview(4)
        d = Driver(eng, 4)
        d.admit([0, 1, 2, 3], [0, 1, 2, 3], 12, FMT)
        d.step(5)
        old = list(d.frames[1])
        eng.cancel_slots([1])
        d.step(gap)
        assert len(d.frames[1]) == len(old)
        start = d.admit([1], [7], 6, {1: NEW_FMT})
        d.step(1)
        pv = eng.fetch_previews(wait=True) if pipeline else []
        d.step(11 + d.lag)
        tag = f"pipeline={pipeline} bf={back_frames} gap={gap}"
        new = d.frames[1][len(old):]
        assert all(x[0] >= start for x in new) and new[0][0] == start, (tag, [x[0] for x in new], start)
        check_frames(oracle, old, 1, 12, False, tag=tag)
        check_frames(oracle, new, 7, 6, True, tag=tag)
        assert [x[4] for x in new] == want, tag
        for b in (0, 2, 3):
            check_frames(oracle, d.frames[b], b, 12, True, tag=tag)
        check_wire(eng, d.frames[0], FMT[0], tag)
        # previews: one per slot at most; slot 1's, if its new utterance's first call has run, is the new one's
        slots = [s for s, _ in pv]
        assert len(set(slots)) == len(slots), (tag, slots)
        for s, pcm in pv:
            ref = oracle_frames(oracle, 7 if s == 1 else s, 1)[0]["pcm"]
            assert pcm_err(pcm - ref) <= PCM_TOL, (tag, s)
        if pipeline and start == d.k - 12 - d.lag:  # the new row started in the call before the fetch
            assert 1 in slots, tag
    finally:
        eng.close()


@pytest.mark.parametrize("back_frames", [1, 2, 4])
def test_previous_utterance_in_flight_is_not_masked(oracle, back_frames):
    """A driver with one call in flight. Slot 0's 4-frame utterance A has frames in flight and
    unfetched when B is admitted into the slot, and B is cancelled two calls later: A's frames
    (calls before B's admission) all still arrive, the last one flagged; B's frames in flight at
    the cancel (calls from its admission on) never do."""
    eng = engine((True, back_frames), wire=False)
    try:
        d = Driver(eng, 1)

        def call():
            eng.step_async(1)
            d.k += 1
            if d.k > 1:
                d.take(1)

        d.admit([0], [0], 4)
        for _ in range(5):  # the fifth call launches the pass over A's last frame
            call()
        assert len(d.frames[0]) < 4
        admitted = d.k
        d.admit([0], [1], 6)
        call()
        call()
        in_flight = 4 - len(d.frames[0])
        eng.cancel_slots([0])
        for _ in range(8 + d.lag):
            call()
        if back_frames > 1:
            assert in_flight > 0  # some of A's frames came only after B's cancel
        assert all(f[0] < admitted for f in d.frames[0])
        check_frames(oracle, d.frames[0], 0, 4, True, tag=f"bf={back_frames}")
    finally:
        eng.close()


@pytest.mark.parametrize("pipeline,back_frames", [(False, 1), (True, 2)])
def test_cancelled_row_stops_counting_euler_steps(oracle, pipeline, back_frames):
    """Cap 4; row 0 runs 1 Euler step, row 1 runs 4. Once row 1 is cancelled the batch runs 1."""
    eng = engine((pipeline, back_frames), wire=False, max_lsd_steps=4)
    try:
        d = Driver(eng, 2)
        d.admit([0, 1], [0, 1], 8, lsd={0: 1, 1: 4})
        d.step(3)
        assert eng.lsd_steps() == (4, 4)
        eng.cancel_slots([1])
        for _ in range(5 + d.lag):
            d.step(1)
            assert eng.lsd_steps() == (4, 1)
        check_frames(oracle, d.frames[0], 0, 8, True, lsd=1)
        check_frames(oracle, d.frames[1], 1, 8, False, lsd=4)
        assert all(f[0] < 3 for f in d.frames[1])
    finally:
        eng.close()


def test_row_cancelled_before_it_starts(oracle):
    """Four-frame passes: a row admitted inside a pass waits for the pass boundary; cancelled before
    it, it never yields a frame."""
    eng = engine((True, 4), wire=False)
    try:
        d = Driver(eng, 2)
        d.admit([0], [0], 10)
        d.step(1)
        start = d.admit([1], [1], 10)
        assert start == 4 and eng.frame_lag()[1] == 3
        d.step(1)
        eng.cancel_slots([1])
        d.step(16)
        assert d.frames[1] == []
        check_frames(oracle, d.frames[0], 0, 10, True)
    finally:
        eng.close()


@pytest.mark.parametrize("pipeline,back_frames", [(False, 1), (True, 2)])
def test_argument_checks_cancel_nothing(oracle, pipeline, back_frames):
    import pocket_tts_amd as pt

    eng = engine((pipeline, back_frames), wire=False)
    try:
        d = Driver(eng, 4)
        eng.cancel_slots([3])  # never admitted: a no-op
        eng.cancel_slots([])
        d.admit([0, 1, 2], [0, 1, 2], 3)
        for bad in ([1, 4], [-1], [1, 2, 1]):
            with pytest.raises(pt.PocketTTSError) as e:
                eng.cancel_slots(bad)
            assert e.value.code == 1, bad
        d.step(3 + d.lag)
        for b in (0, 1, 2):  # nothing was cancelled: every row delivers all its frames
            check_frames(oracle, d.frames[b], b, 3, True)
        eng.cancel_slots([0, 3])  # finished / idle: no-ops
        d.admit([0], [2], 2)
        d.step(2 + d.lag + eng.frame_lag()[1])
        check_frames(oracle, d.frames[0][3:], 2, 2, True)
    finally:
        eng.close()


def test_scheduler_cancels_a_group_on_the_real_engine(oracle):
    """BatchScheduler on a pipelined engine (frame-pair passes, previews on): a group of 5 segments
    at 2 segment rows beside two plain requests, cancelled once its second segment and the pause
    behind it have been delivered. The plain requests and what the group delivered are
    oracle-exact and in order, and the scheduler ends empty."""
    from pocket_tts_amd.serve import BatchScheduler

    eng = engine((True, 2), wire=False)
    sch = BatchScheduler(eng, segment_rows=2)
    try:
        voices = sch.call(lambda: [eng.voice_from_prompt(utterance(u)[0]) for u in (0, 1, 20)])
        lens = [4, 3, 60, 60, 60]
        segs = [("text", utterance(20 + i)[1], params(n)) for i, n in enumerate(lens)]
        segs.insert(2, ("pause", 10))
        with sch.cv:
            g = sch.submit_group(segs, voices[2])
            plain = [sch.submit(utterance(u)[1], voices[u], params(12)) for u in (0, 1)]
        got = []
        for x in g.stream(timeout=60):
            got.append(x)
            if len(got) == 4 + 3 + 1:
                g.cancel()
        assert len(got) >= 8 and got[7].shape == (240,) and not got[7].any()
        frames = got[:7] + got[8:]
        assert all(x.shape == (1920,) for x in frames) and len(frames) < 7 + 60
        want = (oracle_frames(oracle, 20, 4, voice=20) + oracle_frames(oracle, 21, 3, voice=20)
                + oracle_frames(oracle, 22, len(frames) - 7, voice=20))
        for i, (x, ref) in enumerate(zip(frames, want)):
            assert pcm_err(x - ref["pcm"]) <= PCM_TOL, ("group", i)
        for u, r in zip((0, 1), plain):
            fr = list(r.stream(timeout=60))
            assert len(fr) == 12
            for i, (x, ref) in enumerate(zip(fr, oracle_frames(oracle, u, 12))):
                assert pcm_err(x - ref["pcm"]) <= PCM_TOL, (u, i)
        sch.call(lambda: None)
        assert sch.load() == 0 and not sch.active and not sch.waiting and not g.pending
        print(f"group: {len(frames)} frames delivered, {len(frames) - 7} of segment 2")
    finally:
        sch.close()
        eng.close()
