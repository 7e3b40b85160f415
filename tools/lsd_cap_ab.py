"""Cost of the per-row LSD count when unused: a cap-1 engine against a cap-4 engine whose rows all
use n = 1 (lsd_run = 1 in both). Bench-shaped job: B = 32, pipelined, back_frames = 4, 125-frame
prompt, 40 tokens. Alternates the two configurations, 3 rounds; prints one JSON line each
(profiles/lsd_rows/cap1_vs_cap4.txt). Run from anywhere: python tools/lsd_cap_ab.py"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1] / "pocket-tts_amd"))
import pocket_tts_amd as pt  # noqa: E402

B, F, T, K = 32, 125, 40, 125
WARM, STEPS = 12, 100
rng = np.random.default_rng(0)
prompt = (0.1 * rng.standard_normal((F, 1024))).astype(np.float32)
ids = [rng.integers(0, 4000, size=T).astype(np.int32) for _ in range(B)]


def run(cap):
    eng = pt.Engine(device=0, max_slots=B, max_ctx=F + T + K + 8, lsd_decode_steps=1, max_lsd_steps=cap, seed=0x5EED,
                    pipeline=True, back_frames=4)
    try:
        v = eng.voice_from_prompt(prompt)
        ps = [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=K, seed=100 + b, lsd_steps=1)
              for b in range(B)]
        eng.open_many(list(range(B)), [v] * B, ids, ps)
        for _ in range(WARM):
            eng.step_async(B)
            eng.fetch(B)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            eng.step_async(B)
            eng.fetch(B)
        eng.sync()
        el = time.perf_counter() - t0
        capq, last = eng.lsd_steps()
        chain = eng.time_kernel(B, "head.chain", reps=300)
        prelude = eng.time_kernel(B, "head.prelude", reps=300)
        return {"cap": capq, "last_run": last, "steady_ms_per_step": round(1000 * el / STEPS, 4),
                "head_chain_us": round(chain, 3), "head_prelude_us": round(prelude, 3)}
    finally:
        eng.close()


for rnd in range(3):
    for cap in (1, 4):
        r = run(cap)
        r["round"] = rnd
        print(json.dumps(r), flush=True)
