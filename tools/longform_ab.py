"""Measurements behind DESIGN.md section 18 (long-form requests on parallel rows, cancel without a
drain). One box, arms interleaved, 3 rounds; one JSON line per run.

  python tools/longform_ab.py text     (a) the long text of bench.py's text benchmark ("The quick brown
        fox ..." x 10, ref.wav voice, synthetic vocabulary, temp 0, no EOS and the default EOS):
        generate_with_pauses on a one-slot sequential engine (the sequential path, which this work
        leaves as it was) against generate_parallel(pauses=True) at max_slots 8 and 32 (pipelined,
        frame-pair passes): wall time and x real time.
  python tools/longform_ab.py cancel   (b) pipelined engine, B = 32, four-frame passes, 8 calls queued
        and unfetched: how long ptts_slots_cancel of one row and ptts_slot_close of one row take to
        return; and the steady step time with and without one cancel + re-admission every 16 calls.

(c), the HTTP load of tools/serve_load.py with three-sentence long_form requests, needs a server
with a tokenizer behind the load generator and is not scripted here."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pocket-tts_amd"))
import pocket_tts_amd as pt  # noqa: E402

LONG_TEXT = "The quick brown fox jumps over the lazy dog. " * 10


def tokenizer():
    from pocket_tts_amd.text import Metaspace, Tokenizer, Unigram

    g = json.load(open(ROOT / "tests" / "golden" / "text_ids.json"))["synthetic"]
    return Tokenizer(Unigram([tuple(v) for v in g["vocab"]], g["unk_id"], True), Metaspace())


def ref_voice_samples():
    import wave

    with wave.open(str(ROOT / "tests" / "golden" / "ref.wav"), "rb") as w:
        x = np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.float32) / 32768.0
        return x, w.getframerate()


def gen(name, m, v):
    if name.startswith("seq"):
        return m.generate_with_pauses(LONG_TEXT, v)
    return m.generate_parallel(LONG_TEXT, v, pauses=True)


def text_arms(rounds=3):
    tok = tokenizer()
    x, sr = ref_voice_samples()
    arms = [("sequential_1slot", dict(max_slots=1)), ("parallel_8", dict(max_slots=8, pipeline=True, back_frames=2)),
            ("parallel_32", dict(max_slots=32, pipeline=True, back_frames=2))]
    models = []
    for name, kw in arms:
        m = pt.TTSModel.load_with_params(temp=0.0, eos_threshold=float("inf"), tokenizer=tok, max_ctx=1024, **kw)
        models.append((name, m, m.get_voice_state_from_tensor(x, sr)))
    try:
        for eos_name, thr in (("no_eos", float("inf")), ("eos_default", -4.0)):
            for name, m, v in models:  # warm: the graphs of every row count
                m.eos_threshold = thr
                gen(name, m, v)
            for rnd in range(rounds):
                for name, m, v in models:
                    m.engine.sync()
                    t = time.perf_counter()
                    a = gen(name, m, v)
                    wall = time.perf_counter() - t
                    audio_s = a.shape[-1] / 24000.0
                    print(json.dumps({"part": "text", "eos": eos_name, "arm": name, "round": rnd,
                                      "segments": len(m.split_into_best_sentences(LONG_TEXT)),
                                      "audio_s": round(audio_s, 2), "wall_ms": round(1000 * wall, 2),
                                      "x_real_time": round(audio_s / wall, 1)}), flush=True)
    finally:
        for _, m, _ in models:
            m.engine.close()


B, F, T, K = 32, 125, 40, 400


def bench_engine():
    rng = np.random.default_rng(0)
    eng = pt.Engine(device=0, max_slots=B, max_ctx=F + T + K + 8, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                    back_frames=4)
    v = eng.voice_from_prompt((0.1 * rng.standard_normal((F, 1024))).astype(np.float32))
    ids = [rng.integers(0, 4000, size=T).astype(np.int32) for _ in range(B)]
    ps = [pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=K, seed=100 + b) for b in range(B)]
    eng.open_many(list(range(B)), [v] * B, ids, ps)
    return eng, v, ids, ps


def cancel_arms(rounds=3):
    for rnd in range(rounds):
        for arm in ("slots_cancel", "slot_close"):  # 8 calls queued, nothing fetched
            eng, v, ids, ps = bench_engine()
            try:
                for _ in range(16):
                    eng.step_async(B)
                eng.sync()
                for _ in range(8):
                    eng.step_async(B)
                t = time.perf_counter()
                if arm == "slots_cancel":
                    eng.cancel_slots([5])
                else:
                    eng.close_slot(5)
                ret = time.perf_counter() - t
                t = time.perf_counter()
                eng.sync()
                drain = time.perf_counter() - t
                print(json.dumps({"part": "cancel_return", "arm": arm, "round": rnd, "return_us": round(1e6 * ret, 1),
                                  "sync_after_us": round(1e6 * drain, 1)}), flush=True)
            finally:
                eng.close()
        for arm in ("steady", "cancel_readmit_every_16"):
            eng, v, ids, ps = bench_engine()
            try:
                def call(i, first=False):
                    if arm != "steady" and i % 16 == 8:
                        s = (i // 16) % B
                        eng.cancel_slots([s])
                        eng.open_many([s], [v], [ids[s]], [ps[s]])
                    eng.step_async(B)
                    if not first:
                        eng.fetch(B, calls_back=1)

                for i in range(32):
                    call(i, i == 0)
                eng.sync()
                steps = 160
                t = time.perf_counter()
                for i in range(32, 32 + steps):
                    call(i)
                eng.sync()
                el = time.perf_counter() - t
                print(json.dumps({"part": "cancel_steady", "arm": arm, "round": rnd,
                                  "steady_ms_per_step": round(1000 * el / steps, 4)}), flush=True)
            finally:
                eng.close()


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "all"
    if part in ("text", "all"):
        text_arms()
    if part in ("cancel", "all"):
        cancel_arms()
