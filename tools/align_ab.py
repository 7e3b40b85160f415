"""Cost of the align stage: a bench-shaped job (B = 32, pipelined, 125-frame
prompt, 40 tokens, four-frame passes) on an engine without the stage, on an align-enabled engine
whose rows ask for nothing, and with all 32 rows in the stage at S = 40 (layer 0, all 16 heads). The
launch sits on the front chain, so the steady step is what it costs. The driver keeps one call in
flight and fetches every frame and, for rows in the stage, every alignment row, as the server does.
Alternates the arms, 3 rounds; one JSON line per run: steady ms per step and the flow.l<L>.align
launch's own time (ptts_time_kernel over the rows, mid-utterance), then the medians.
python tools/align_ab.py [back_frames] [layer] [head mask]"""
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
LAYER = int(sys.argv[2]) if len(sys.argv) > 2 else 0
HEADS = int(sys.argv[3], 0) if len(sys.argv) > 3 else 0xFFFF
# (name, align stage, rows in it)
ARMS = [("no_stage", False, False), ("enabled_unused", True, False), ("all_rows_s40", True, True)]
rng = np.random.default_rng(0)
prompt = (0.1 * rng.standard_normal((F, 1024))).astype(np.float32)
ids = [rng.integers(0, 4000, size=T).astype(np.int32) for _ in range(B)]


def run(name, stage, rows):
    kw = dict(align=True, align_layer=LAYER, align_heads=HEADS) if stage else {}
    eng = pt.Engine(device=0, max_slots=B, max_ctx=F + T + K + 8, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                    back_frames=BF, **kw)
    try:
        v = eng.voice_from_prompt(prompt)
        ps = [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=K, seed=100 + b) for b in range(B)]
        for p in ps:
            p.align = rows
        eng.open_many(list(range(B)), [v] * B, ids, ps)
        got = 0

        def call(first):
            nonlocal got
            eng.step_async(B)
            if not first:
                eng.fetch(B, calls_back=1)
                if rows:
                    got += sum(a.size for a in eng.fetch_align(B, calls_back=1))

        for i in range(WARM):
            call(i == 0)
        eng.sync()
        got = 0
        t0 = time.perf_counter()
        for _ in range(STEPS):
            call(False)
        eng.sync()
        el = time.perf_counter() - t0
        out = {"arm": name, "back_frames": BF, "steady_ms_per_step": round(1000 * el / STEPS, 4),
               "align_floats_per_step": got // STEPS}
        if stage:
            out["align_launch_us"] = round(eng.time_kernel(B, f"flow.l{LAYER}.align", reps=100), 3)
        out["attention_launch_us"] = round(eng.time_kernel(B, f"flow.l{LAYER}.attention", reps=100), 3)
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
    for key in ("steady_ms_per_step", "align_launch_us", "attention_launch_us", "align_floats_per_step"):
        if key in mine[0]:
            med[key] = statistics.median(r[key] for r in mine)
    print(json.dumps(med), flush=True)
