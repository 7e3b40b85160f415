"""back_frames = 8, the widest back pass the engine accepts (NFR_MAX; pocket_tts.h and
INTEGRATION.md document it), against the oracle: 128 ring positions appended ahead of each Mimi
attention, passes of 8 frames with partial tails, a frame arriving 15 calls after the call that
computed it. Rows of 3 frames (one partial pass), 13 (a full pass and a partial one) and 40 (five
full passes: the 512-position ring wraps) share the batch; temp 0, the backbone input teacher-forced
to the oracle's latent so that per-step differences do not compound over 40 autoregressive steps.
The 13-frame row carries a wire format: the wire block is laid out per pass, and its chunks must
concatenate bit for bit to the encoding of its whole PCM (test_gpu_wire.check_rows)."""

import numpy as np
import pytest
from conftest import LAT_TOL, PCM_TOL, load_golden, pcm_err
from test_gpu_wire import check_rows, params

pytestmark = pytest.mark.gpu


def test_back_frames_8_matches_oracle(oracle):
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(8)
    frames = [3, 13, 40]
    formats = [None, (44100, "pcm_s16le"), None]
    eng = pt.Engine(device=0, max_slots=3, max_ctx=128, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                    back_frames=8, wire=True)
    try:
        want, vs, ids_l = [], [], []
        for b in range(3):
            F = 6 + 2 * b
            prompt = (d["prompt"][:F] * (1.0 + 0.05 * b)).astype(np.float32)
            ids = rng.integers(0, 4000, size=4 + 3 * b).astype(np.int32)
            vs.append(eng.voice_from_prompt(prompt))
            ids_l.append(ids)
            s = oracle.new_state(128)
            s.prefill(prompt)
            s.prefill_tokens(ids)
            lat, out = None, []
            for _ in range(frames[b]):
                out.append(s.step(lat))
                lat = out[-1]["latent"]
            want.append(out)
        eng.open_many([0, 1, 2], vs, ids_l, [params(frames[b], formats[b]) for b in range(3)])
        assert eng.frame_lag() == (15, 0)  # admitted at call 0, a pass boundary
        got = [0] * 3
        pcm = [[] for _ in range(3)]
        wire = [[] for _ in range(3)]
        worst_lat = worst_pcm = 0.0
        for call in range(max(frames) + 15):
            if call < max(frames):
                eng.step_async(3)
                for b in range(3):
                    if call < frames[b]:  # the front part of this call computed the row's frame `call`
                        eng.set_latent(b, want[b][call]["latent"])
            else:
                eng.flush_async(3)
            r = eng.fetch(3)
            w = eng.fetch_wire(3)
            assert not r.valid.any() or call >= 15
            for b in range(3):
                if not r.valid[b]:
                    assert w[b] == b"", (call, b)
                    continue
                o = want[b][got[b]]
                got[b] += 1
                assert got[b] <= frames[b] and bool(r.last[b]) == (got[b] == frames[b]), (call, b, got[b])
                assert abs(r.eos_logits[b] - o["eos_logit"]) <= LAT_TOL, (call, b)
                np.testing.assert_allclose(r.latents[b], o["latent"], atol=LAT_TOL)
                worst_lat = max(worst_lat, float(np.abs(r.latents[b] - o["latent"]).max()))
                e = pcm_err(r.pcm[b] - o["pcm"])
                assert e <= PCM_TOL, (call, b, got[b], e)
                worst_pcm = max(worst_pcm, e)
                pcm[b].append(r.pcm[b].copy())
                wire[b].append(w[b])
        assert got == frames, got
        print(f"back_frames=8: worst latent |d| {worst_lat:.3g}, worst PCM |d| {worst_pcm:.3g}")
        check_rows(eng, formats, frames, pcm, wire, "back_frames=8")
    finally:
        eng.close()
