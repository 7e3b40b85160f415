"""Measurement behind DESIGN.md section 20 (rows admitted behind a teacher-forced latent prefix).
One box, arms interleaved, 3 rounds; one JSON line per run.

  python tools/continuation_ab.py [sequential|pipelined]
        32 rows, a 125-frame voice, 80 tokens and a 100-frame prefix per row. Two ways of getting the
        first NEW frame of every row onto the host, each timed from the admission call:
          prefix_admission   ptts_slots_open_opts with the prefix, then steps until the frame arrives;
          forced_steps       the admission without the prefix, then 100 steps with every row's sampled
                             latent replaced through ptts_slot_set_latent (the only way before), then
                             the step that computes the new frame;
          free_steps         as forced_steps without the set_latent calls (its 101 steps alone: the
                             floor of any step-at-a-time scheme; the frames are not the forced ones).
        The pipelined engine (frame-pair passes) is the server's configuration; its frames trail
        their step by frame_lag() calls.

bench.py at its default against the parent commit is run by hand on the same box (both trees built,
three interleaved rounds); its record lies beside this tool's in profiles/continuation/."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pocket-tts_amd"))
import pocket_tts_amd as pt  # noqa: E402

B, F, S, NP, NEW = 32, 125, 80, 100, 4


def first_frame(eng, t0):
    """Step until every row has returned a frame; ms since t0."""
    seen = np.zeros(B, bool)
    for _ in range(16):
        eng.step_async(B)
        seen |= eng.fetch(B).valid
        if seen.all():
            return 1000 * (time.perf_counter() - t0)
    raise RuntimeError("no first frame")


def drain(eng):
    for _ in range(NEW + 8):
        eng.step_async(B)
        eng.fetch(B)
    eng.sync()


def run(kind, rounds=3):
    rng = np.random.default_rng(0)
    kw = dict(pipeline=True, back_frames=2) if kind == "pipelined" else {}
    eng = pt.Engine(device=0, max_slots=B, max_ctx=F + S + NP + NEW + 8, lsd_decode_steps=1, seed=0x5EED, **kw)
    try:
        v = eng.voice_from_prompt((0.1 * rng.standard_normal((F, 1024))).astype(np.float32))
        ids = [rng.integers(0, 4000, size=S).astype(np.int32) for _ in range(B)]
        pre = [rng.standard_normal((NP, 32)).astype(np.float32) for _ in range(B)]
        slots = list(range(B))

        def params(with_prefix, frames):
            return [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=frames, seed=100 + b,
                                        prefix_latents=pre[b] if with_prefix else None) for b in range(B)]

        def arm(name):
            eng.sync()
            t0 = time.perf_counter()
            if name == "prefix_admission":
                eng.open_many(slots, [v] * B, ids, params(True, NEW))
                return first_frame(eng, t0)
            eng.open_many(slots, [v] * B, ids, params(False, NP + NEW))
            for j in range(NP):
                eng.step_async(B)
                if name == "forced_steps":
                    for b in range(B):
                        eng.set_latent(b, pre[b][j])
            # the frames of the forced steps are discarded; the next valid one is the first new frame
            eng.sync()
            eng.fetch(B)
            return first_frame(eng, t0)

        arms = ("prefix_admission", "forced_steps", "free_steps")
        for name in arms:  # warm: graphs, first-use allocations
            arm(name)
            drain(eng)
        for rnd in range(rounds):
            for name in arms:
                ms = arm(name)
                drain(eng)
                print(json.dumps({"engine": kind, "arm": name, "round": rnd, "rows": B, "voice_frames": F, "tokens": S,
                                  "prefix_frames": NP, "first_new_frame_ms": round(ms, 3)}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    for kind in (sys.argv[1:] or ["sequential", "pipelined"]):
        run(kind)
