"""Cost of the level stage: a bench-shaped job (B = 32, pipelined, 125-frame
prompt, 40 tokens, four-frame passes) on an engine with the tempo and pitch stages and no level
stage, on a level-enabled engine whose rows ask for nothing, and with all rows at +6 dB as 16-bit
@ 24 kHz, as 16-bit @ 48 kHz, and at speed 0.8, pitch +4 and +6 dB as 16-bit @ 48 kHz. The ceiling
is -26 dBFS, which the synthetic weights' PCM (peaks near 0.053) crosses at +6 dB in most samples,
so the limiter works in every frame. The driver keeps one call in flight and fetches every frame
and, for wire rows, every chunk, as the server does. Alternates the arms, 3 rounds; one JSON line per
run: steady ms per step, and the tempo, pitch, level and wire launches' own times (ptts_time_kernel
over the pass's rows, mid-utterance), then the medians.
python tools/level_ab.py [back_frames]"""
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1] / "pocket-tts_amd"))
import pocket_tts_amd as pt  # noqa: E402

B, F, T, K = 32, 125, 40, 200
WARM, STEPS = 16, 120
BF = int(sys.argv[1]) if len(sys.argv) > 1 else 4
CEILING_DB = -26.0
# (name, level stage, (rate, encoding), volume in dB, speed, pitch in semitones)
ARMS = [("no_level", False, None, None, None, None), ("enabled_unused", True, None, None, None, None),
        ("p6db_s16_24k", True, (24000, "pcm_s16le"), 6.0, None, None),
        ("p6db_s16_48k", True, (48000, "pcm_s16le"), 6.0, None, None),
        ("p6db_sp800_p400_s16_48k", True, (48000, "pcm_s16le"), 6.0, 0.8, 4.0)]
rng = np.random.default_rng(0)
prompt = (0.1 * rng.standard_normal((F, 1024))).astype(np.float32)
ids = [rng.integers(0, 4000, size=T).astype(np.int32) for _ in range(B)]


def run(name, level, fmt, volume_db, speed, semitones):
    kw = dict(level=True, level_ceiling_db=CEILING_DB) if level else {}
    eng = pt.Engine(device=0, max_slots=B, max_ctx=F + T + K + 8, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                    back_frames=BF, wire=True, tempo=True, pitch=True, **kw)
    try:
        v = eng.voice_from_prompt(prompt)
        ps = [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=K, seed=100 + b) for b in range(B)]
        for p in ps:
            if fmt:
                p.sample_rate, p.encoding = fmt
            p.volume_db, p.speed, p.pitch = volume_db, speed, semitones
        eng.open_many(list(range(B)), [v] * B, ids, ps)
        nbytes = 0

        def call(first):
            nonlocal nbytes
            eng.step_async(B)
            if not first:
                eng.fetch(B, calls_back=1)
                if fmt:
                    nbytes += sum(len(c) for c in eng.fetch_wire(B, calls_back=1))

        for i in range(WARM):
            call(i == 0)
        eng.sync()
        nbytes = 0
        t0 = time.perf_counter()
        for _ in range(STEPS):
            call(False)
        eng.sync()
        el = time.perf_counter() - t0
        out = {"arm": name, "back_frames": BF, "steady_ms_per_step": round(1000 * el / STEPS, 4),
               "wire_bytes_per_step": nbytes // STEPS}
        # the launches alone over one pass of the rows' current frames (they advance the rows' state)
        out["tempo_launch_us"] = round(eng.time_kernel(B, "tempo", reps=100), 3)
        out["pitch_launch_us"] = round(eng.time_kernel(B, "pitch", reps=100), 3)
        if level:
            out["level_launch_us"] = round(eng.time_kernel(B, "level", reps=100), 3)
        out["wire_launch_us"] = round(eng.time_kernel(B, "wire", reps=100), 3)
        return out
    finally:
        eng.close()


runs = []
for rnd in range(3):
    for arm in ARMS:
        r = run(*arm)
        r["round"] = rnd
        runs.append(r)
        print(json.dumps(r), flush=True)
for name, *_ in ARMS:
    mine = [r for r in runs if r["arm"] == name]
    med = {"arm": name, "median_of": len(mine)}
    for key in ("steady_ms_per_step", "tempo_launch_us", "pitch_launch_us", "level_launch_us", "wire_launch_us",
                "wire_bytes_per_step"):
        if key in mine[0]:
            med[key] = statistics.median(r[key] for r in mine)
    print(json.dumps(med), flush=True)
