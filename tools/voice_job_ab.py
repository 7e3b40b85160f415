"""Cost of cloning a voice while the engine streams: one pipelined engine (back_frames = 2) with 32
rows generating, and a 15-s clip (tests/golden/ref.wav, 48 kHz int16, repeated to 15 s) cloned once
every 50 calls. Per case, the median and the maximum wall time of a call (step_async + fetch, the
clone's own host time included in the call that makes it):

  a  no cloning
  b  voice_from_audio (synchronous: drains the pipeline; the samples converted on the host)
  c  voice_job (the voice stream; int16 samples converted on the GPU)
  d  voice_job, and each clone's call also destroys the voice made three clones earlier (a server
     whose cache is evicting: ptts_voice_destroy frees device and pinned memory on the caller's thread)

and, on an idle engine, the submit-to-ready time of a lone job beside the synchronous call.

The driver (no arguments) touches no GPU itself: it runs every case as a child process under its
own `timeout -k 10`, the cases interleaved over --rounds rounds, and stops at the first non-zero
status. One JSON line per run (profiles/voice_jobs/).
Run from anywhere: python tools/voice_job_ab.py"""
import argparse
import json
import subprocess
import sys
import time
import wave
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
B, T = 32, 40
WARM, CALLS, EVERY = 12, 400, 50
CLIP_S = 15


def clip_i16():
    with wave.open(str(ROOT / "tests" / "golden" / "ref.wav"), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48000)
        x = np.frombuffer(w.readframes(w.getnframes()), np.int16)
    n = CLIP_S * 48000
    return np.ascontiguousarray(np.tile(x, n // x.size + 1)[:n])


def engine(pt, slots, ctx):
    return pt.Engine(device=0, max_slots=slots, max_ctx=ctx, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                     back_frames=2)


def run_case(case):
    sys.path.insert(0, str(ROOT / "pocket-tts_amd"))
    import pocket_tts_amd as pt

    x = clip_i16()
    frames = (CLIP_S * 24000 + 1919) // 1920
    rng = np.random.default_rng(0)
    if case == "lone":
        eng = engine(pt, 1, frames + 64)
        try:
            eng.reserve_voice_jobs(frames)
            job, sync = [], []
            for _ in range(6):
                t0 = time.perf_counter()
                v = eng.voice_job(x, 48000)
                t1 = time.perf_counter()
                v.ready(wait=True)
                t2 = time.perf_counter()
                v.close()
                job.append((1e3 * (t1 - t0), 1e3 * (t2 - t0)))
                t0 = time.perf_counter()
                w = eng.voice_from_audio(x.astype(np.float32) / np.float32(32768.0), 48000)
                sync.append(1e3 * (time.perf_counter() - t0))
                w.close()
            job, sync = job[1:], sync[1:]  # the first of each warms the code objects
            return {"case": "lone", "frames": frames, "job_submit_ms": round(float(np.median([j[0] for j in job])), 3),
                    "job_submit_to_ready_ms": round(float(np.median([j[1] for j in job])), 3),
                    "voice_from_audio_ms": round(float(np.median(sync)), 3)}
        finally:
            eng.close()
    K = WARM + CALLS + 16
    eng = engine(pt, B, frames + T + K + 8)
    try:
        eng.reserve_voice_jobs(frames)
        prompt = (0.1 * rng.standard_normal((125, 1024))).astype(np.float32)
        ids = [rng.integers(0, 4000, size=T).astype(np.int32) for _ in range(B)]
        v0 = eng.voice_from_prompt(prompt)
        if case != "a":  # warm the clone path's code objects outside the measurement
            (eng.voice_from_audio(x[:48000].astype(np.float32) / np.float32(32768.0), 48000) if case == "b"
             else eng.voice_job(x[:48000], 48000)).close()
        ps = [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=K, seed=100 + b) for b in range(B)]
        eng.open_many(list(range(B)), [v0] * B, ids, ps)
        for _ in range(WARM):
            eng.step_async(B)
            eng.fetch(B)
        voices, ms, clone_calls = [], [], []
        for k in range(CALLS):
            t0 = time.perf_counter()
            if case != "a" and k % EVERY == EVERY // 2:
                clone_calls.append(k)
                if case == "b":
                    voices.append(eng.voice_from_audio(x.astype(np.float32) / np.float32(32768.0), 48000))
                else:
                    voices.append(eng.voice_job(x, 48000))
                    if case == "d" and len(voices) > 3:
                        voices[-4].close()
            eng.step_async(B)
            r = eng.fetch(B)
            ms.append(1e3 * (time.perf_counter() - t0))
            assert r.valid.all()
        eng.sync()
        for v in voices:
            if v.handle is not None:
                assert v.ready(wait=True) and v.n_frames == frames
                v.close()
        ms = np.array(ms)
        near = np.zeros(CALLS, bool)  # the clone's call and the 7 after it (pipeline refill)
        for k in clone_calls:
            near[k:k + 8] = True
        return {"case": case, "calls": CALLS, "clones": len(clone_calls), "median_ms": round(float(np.median(ms)), 4),
                "p99_ms": round(float(np.percentile(ms, 99)), 4), "max_ms": round(float(ms.max()), 4),
                "sum_ms": round(float(ms.sum()), 2),
                "max_ms_at_clones": round(float(ms[near].max()), 4) if near.any() else None,
                # the clone's call and the 7 after it, averaged over the clones
                "ms_after_clone": [round(float(np.mean([ms[k + d] for k in clone_calls])), 3) for d in range(8)]
                if clone_calls else None}
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("a", "b", "c", "d", "lone"), default=None, help="run one case in this process")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit-s", type=int, default=120, help="time limit of each case's process")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case)), flush=True)
        return 0
    for rnd in range(args.rounds):
        for case in ("a", "b", "c", "d") + (("lone",) if rnd == 0 else ()):
            rc = subprocess.run(["timeout", "-k", "10", str(args.limit_s), sys.executable, __file__, "--case", case]).returncode
            if rc != 0:
                print(f"case {case} (round {rnd}) ended with status {rc}: stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
