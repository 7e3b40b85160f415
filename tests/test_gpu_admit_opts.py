"""The five C admission entry points admit the same row (include/pocket_tts.h: ptts_slot_open,
ptts_slots_open, ptts_slot_open_ex, ptts_slots_open_ex, ptts_slots_open_opts).

Engine.open_many calls ptts_slots_open_opts alone, so this is where the other four, a NULL opts and
the older struct sizes are run: the same (voice, ids, params) on slot 0 through each, stepped to its
last frame, must give bit-identical PCM, latents, EOS logits and valid / last flags. One engine
(the 4-slot, 128-position one of test_gpu_continuation.py), one voice."""

import ctypes as C

import numpy as np
import pytest
from conftest import load_golden

pytestmark = pytest.mark.gpu

FRAMES = 3


def test_entry_points_admit_the_same_row():
    import pocket_tts_amd as pt
    from pocket_tts_amd._lib import SlotOpts, SlotOpts5, check, lib

    L = lib()
    i32 = C.POINTER(C.c_int32)
    ids = np.array([260, 2994, 262, 578], np.int32)
    cp = pt.GenerationParams(temp=0.7, eos_threshold=float("inf"), max_frames=FRAMES, seed=11).to_c()
    eng = pt.Engine(device=0, max_slots=4, max_ctx=128, lsd_decode_steps=1, seed=0x5EED)
    try:
        v = eng.voice_from_prompt(load_golden("e2e_lsd1.safetensors")["prompt"][:5].astype(np.float32))
        e, idp = eng.handle, ids.ctypes.data_as(i32)
        many = (1, (C.c_int32 * 1)(0), (C.c_void_p * 1)(v.handle), idp, (C.c_int32 * 1)(ids.size), C.byref(cp))
        ways = {
            "slot_open": lambda: L.ptts_slot_open(e, 0, v.handle, idp, ids.size, C.byref(cp)),
            "slots_open": lambda: L.ptts_slots_open(e, *many),
            "slot_open_ex 0": lambda: L.ptts_slot_open_ex(e, 0, v.handle, idp, ids.size, C.byref(cp), 0),
            "slots_open_ex NULL": lambda: L.ptts_slots_open_ex(e, *many, None),
            "slots_open_opts NULL": lambda: L.ptts_slots_open_opts(e, *many, None),
            "slots_open_opts 24": lambda: L.ptts_slots_open_opts(e, *many, C.cast((SlotOpts * 1)(SlotOpts(24)), C.c_void_p)),
            "slots_open_opts 64": lambda: L.ptts_slots_open_opts(e, *many, C.cast((SlotOpts5 * 1)(SlotOpts5(64)), C.c_void_p)),
        }
        runs = {}
        for name, admit in ways.items():
            check(admit())
            steps = [eng.step(1) for _ in range(FRAMES)]
            eng.close_slot(0)
            runs[name] = [np.stack([np.array(getattr(r, f)[0]) for r in steps])
                          for f in ("pcm", "latents", "eos_logits", "valid", "last")]
        first = runs["slot_open"]
        assert first[3].all() and list(first[4]) == [False] * (FRAMES - 1) + [True]
        assert np.abs(first[0]).max() > 0 and len({a.tobytes() for a in first[1]}) == FRAMES  # frames differ
        for name, got in runs.items():
            for a, b, what in zip(first, got, ("pcm", "latents", "eos_logits", "valid", "last")):
                assert a.tobytes() == b.tobytes(), (name, what)
    finally:
        eng.close()
