"""Cost of the wire stage: a bench-shaped job (B = 32, pipelined, 125-frame
prompt, 40 tokens) on an engine without wire output, on a wire-enabled engine whose rows ask for no
format, and with all rows 16-bit @ 24 kHz, mu-law @ 8 kHz and 16-bit @ 48 kHz; then with the FLAC stage
(section 21) enabled and unused, and with all rows FLAC @ 24 kHz and @ 48 kHz. The driver keeps one
call in flight and fetches every frame (and, for wire rows, every chunk) as the server does.
Alternates the arms, 3 rounds; one JSON line per run: steady ms per step, and the wire launch's own
time (ptts_time_kernel over the pass's rows, mid-utterance), for the FLAC arms the flac launch's too.
python tools/wire_ab.py [back_frames]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1] / "pocket-tts_amd"))
import pocket_tts_amd as pt  # noqa: E402

B, F, T, K = 32, 125, 40, 200
WARM, STEPS = 16, 120
BF = int(sys.argv[1]) if len(sys.argv) > 1 else 4
ARMS = [("plain", False, None), ("enabled_unused", True, None), ("s16_24k", True, (24000, "pcm_s16le")),
        ("ulaw_8k", True, (8000, "ulaw")), ("s16_48k", True, (48000, "pcm_s16le")),
        ("flac_enabled_unused", "flac", None), ("flac_24k", "flac", (24000, "flac")), ("flac_48k", "flac", (48000, "flac"))]
rng = np.random.default_rng(0)
prompt = (0.1 * rng.standard_normal((F, 1024))).astype(np.float32)
ids = [rng.integers(0, 4000, size=T).astype(np.int32) for _ in range(B)]


def run(name, wire, fmt):
    eng = pt.Engine(device=0, max_slots=B, max_ctx=F + T + K + 8, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                    back_frames=BF, wire=bool(wire), flac=wire == "flac")
    try:
        v = eng.voice_from_prompt(prompt)
        ps = [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=K, seed=100 + b) for b in range(B)]
        if fmt:
            for p in ps:
                p.sample_rate, p.encoding = fmt
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
        if wire:  # the launch alone over one pass of the rows' current frames (advances their wire state)
            out["wire_launch_us"] = round(eng.time_kernel(B, "wire", reps=100), 3)
        if wire == "flac":  # each replay behind a wire launch of its own (the stage overwrites its input)
            out["flac_launch_us"] = round(eng.time_kernel(B, "flac", reps=100), 3)
        return out
    finally:
        eng.close()


for rnd in range(3):
    for arm in ARMS:
        r = run(*arm)
        r["round"] = rnd
        print(json.dumps(r), flush=True)
