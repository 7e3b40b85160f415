"""Cost of the loudness stage: a bench-shaped job (B = 32, pipelined, 125-frame
prompt, 40 tokens, four-frame passes) on a wire-enabled engine with no loudness stage, on a
loudness-enabled engine whose rows ask for nothing, and with all 32 rows metered; every row is
16-bit @ 24 kHz in all three arms, so the arms differ in the meter alone. The driver keeps one call
in flight and fetches every frame, chunk and (third arm) loudness record, as the server does.
Alternates the arms, 3 rounds; one JSON line per run: steady ms per step and the loud and wire
launches' own times (ptts_time_kernel over the pass's rows, mid-utterance), then the medians.
python tools/loud_ab.py [back_frames]"""
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
# (name, loudness stage, rows metered)
ARMS = [("no_loud", False, False), ("enabled_unused", True, False), ("all_metered", True, True)]
rng = np.random.default_rng(0)
prompt = (0.1 * rng.standard_normal((F, 1024))).astype(np.float32)
ids = [rng.integers(0, 4000, size=T).astype(np.int32) for _ in range(B)]


def run(name, loud, metered):
    eng = pt.Engine(device=0, max_slots=B, max_ctx=F + T + K + 8, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                    back_frames=BF, wire=True, **(dict(loud=True) if loud else {}))
    try:
        v = eng.voice_from_prompt(prompt)
        ps = [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=K, seed=100 + b, sample_rate=24000,
                                  encoding="pcm_s16le", loudness=metered) for b in range(B)]
        eng.open_many(list(range(B)), [v] * B, ids, ps)
        nbytes = blocks = 0

        def call(first):
            nonlocal nbytes, blocks
            eng.step_async(B)
            if not first:
                eng.fetch(B, calls_back=1)
                nbytes += sum(len(c) for c in eng.fetch_wire(B, calls_back=1))
                if metered:
                    blocks += sum(e.size for e in eng.fetch_loud(B, calls_back=1))

        for i in range(WARM):
            call(i == 0)
        eng.sync()
        nbytes = blocks = 0
        t0 = time.perf_counter()
        for _ in range(STEPS):
            call(False)
        eng.sync()
        el = time.perf_counter() - t0
        out = {"arm": name, "back_frames": BF, "steady_ms_per_step": round(1000 * el / STEPS, 4),
               "wire_bytes_per_step": nbytes // STEPS, "sub_blocks": blocks}
        # the launches alone over one pass of the rows' current frames (they advance the rows' state)
        if loud:
            out["loud_launch_us"] = round(eng.time_kernel(B, "loud", reps=100), 3)
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
    for key in ("steady_ms_per_step", "loud_launch_us", "wire_launch_us", "wire_bytes_per_step", "sub_blocks"):
        if key in mine[0]:
            med[key] = statistics.median(r[key] for r in mine)
    print(json.dumps(med), flush=True)
