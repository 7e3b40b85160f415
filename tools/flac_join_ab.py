"""Cost of joining FLAC segments on the host: the long text of bench.py's
text benchmark ("The quick brown fox ..." x 10, ref.wav voice, synthetic vocabulary, temp 0, no EOS)
as generate_parallel(pauses=True) on 8 pipelined rows with frame-pair passes, `pcm_s16le` against
`flac`. Arms interleaved, 3 rounds; one JSON line per run: bytes, x real time, and for the FLAC arm
the host time spent in audio.flac_rebase (the ctypes call and its numpy buffers) and the frames it
renumbered. Then ptts_flac_rebase alone over the chunks of the last run (buffers made once, 50
passes): ns per frame and per byte.
python tools/flac_join_ab.py [rate]"""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pocket-tts_amd"))
import pocket_tts_amd as pt  # noqa: E402
from pocket_tts_amd import _lib, audio  # noqa: E402

sys.path.insert(0, str(ROOT / "tools"))
from longform_ab import LONG_TEXT, ref_voice_samples, tokenizer  # noqa: E402

RATE = int(sys.argv[1]) if len(sys.argv) > 1 else 24000
spent = {"s": 0.0, "frames": 0, "calls": []}
_rebase = audio.flac_rebase


def timed_rebase(chunk, index, delta):
    t = time.perf_counter()
    out = _rebase(chunk, index, delta)
    spent["s"] += time.perf_counter() - t
    spent["frames"] += len(index)
    spent["calls"].append((bytes(chunk), list(index), int(delta)))
    return out


audio.flac_rebase = timed_rebase


def main(rounds=3):
    x, sr = ref_voice_samples()
    m = pt.TTSModel.load_with_params(temp=0.0, eos_threshold=float("inf"), tokenizer=tokenizer(), max_ctx=1024, max_slots=8,
                                     pipeline=True, back_frames=2, wire=True, flac=True)
    try:
        v = m.get_voice_state_from_tensor(x, sr)
        for enc in ("pcm_s16le", "flac"):  # warm: the graphs of every row count
            m.generate_parallel(LONG_TEXT, v, pauses=True, sample_rate=RATE, encoding=enc)
        for rnd in range(rounds):
            for enc in ("pcm_s16le", "flac"):
                spent.update(s=0.0, frames=0, calls=[])
                m.engine.sync()
                t = time.perf_counter()
                a = m.generate_parallel(LONG_TEXT, v, pauses=True, sample_rate=RATE, encoding=enc)
                wall = time.perf_counter() - t
                n = int.from_bytes(a[18:26], "big") & ((1 << 36) - 1) if enc == "flac" else len(a) // 2
                r = {"arm": enc, "round": rnd, "rate": RATE, "bytes": len(a), "audio_s": round(n / RATE, 2),
                     "wall_ms": round(1000 * wall, 2), "x_real_time": round(n / RATE / wall, 1)}
                if enc == "flac":
                    r.update(rebase_ms=round(1000 * spent["s"], 3), rebase_frames=spent["frames"],
                             rebase_us_per_frame=round(1e6 * spent["s"] / max(spent["frames"], 1), 2))
                print(json.dumps(r), flush=True)
    finally:
        m.engine.close()
    # the C function alone
    L, jobs = _lib.lib(), []
    for chunk, index, delta in spent["calls"]:
        src = np.frombuffer(chunk, np.uint8).copy()
        idx = np.ascontiguousarray(np.asarray(index, np.int32).reshape(-1, 2))
        out = np.zeros(src.size + 6 * idx.shape[0], np.uint8)
        jobs.append((src.ctypes.data_as(_lib.U8P), src.size, idx.ctypes.data_as(_lib.I32P), idx.shape[0], delta,
                     out.ctypes.data_as(_lib.U8P), out.size, src, idx, out))
    n_out = C.c_int(0)
    reps = 50
    t = time.perf_counter()
    for _ in range(reps):
        for a, na, i, ni, d, o, no, *_ in jobs:
            L.ptts_flac_rebase(a, na, i, ni, d, o, no, C.byref(n_out))
    el = time.perf_counter() - t
    frames, nbytes = sum(j[3] for j in jobs), sum(j[1] for j in jobs)
    print(json.dumps({"part": "ptts_flac_rebase alone (ctypes call included)", "frames": frames, "bytes": nbytes,
                      "us_per_frame": round(1e6 * el / reps / max(frames, 1), 3),
                      "ns_per_byte": round(1e9 * el / reps / max(nbytes, 1), 3)}), flush=True)


if __name__ == "__main__":
    main()
