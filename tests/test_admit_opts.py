"""GenerationParams.slot_opts: the one place a row's ptts_slot_opts is built (no GPU, no engine).

Engine.open_many sends every row as the whole 64-byte struct. The table holds the defaults, each
option alone and one row with all of them; every field must be what the accessors give, and must
agree with the five historical layouts (SlotOpts .. SlotOpts5) filled positionally, which is what
open_many sent before it had one path: the smallest layout that held the options in use."""

import ctypes as C

import numpy as np
import pytest
from pocket_tts_amd import GenerationParams
from pocket_tts_amd._lib import SlotOpts, SlotOpts2, SlotOpts3, SlotOpts4, SlotOpts5

PREFIX = np.arange(3 * 32, dtype=np.float32).reshape(3, 32)
DEFAULT_LSD = 2  # the engine's lsd_decode_steps: lsd_steps of a row that names none
ROWS = {
    "defaults": {},
    "lsd": dict(lsd_steps=3),
    "rate": dict(sample_rate=8000),
    "encoding": dict(encoding="ulaw"),
    "speed": dict(speed=1.25),
    "prefix": dict(prefix_latents=PREFIX),
    "keep_codec": dict(keep_codec=True),
    "pitch": dict(pitch=-3.5),
    "gain": dict(volume_db=-6.5),
    "limit": dict(limit=True),
    "align": dict(align=True),
    "everything": dict(lsd_steps=1, sample_rate=44100, encoding="flac", speed=0.8, prefix_latents=PREFIX,
                       keep_codec=True, pitch=2.0, volume_db=12.0, limit=True, align=True),
}


def expected(p):
    """Field values from the accessors, in the order of SlotOpts5's fields behind `size`."""
    pre = p.prefix()
    lsd = DEFAULT_LSD if p.lsd_steps is None else p.lsd_steps
    return [lsd, *p.opts(), None if pre is None else pre.ctypes.data, 0 if pre is None else pre.shape[0],
            int(p.keep_codec), p.cents(), 0, *p.level(), int(p.align), 0]


@pytest.mark.parametrize("name", list(ROWS))
def test_slot_opts_fields(name):
    p = GenerationParams(**ROWS[name])
    o = p.slot_opts(DEFAULT_LSD)
    assert isinstance(o, SlotOpts5) and C.sizeof(o) == 64 and o.size == 64
    want = expected(p)
    names = [f for f, _ in SlotOpts5._fields_[1:]]
    assert len(names) == len(want)
    for f, w in zip(names, want):
        if f == "prefix_latents":  # the prefix is a fresh contiguous copy: compare what it points to
            if w is None:
                assert o.prefix_latents is None
            else:
                got = np.ctypeslib.as_array(C.cast(o.prefix_latents, C.POINTER(C.c_float)), shape=(o.n_prefix, 32))
                assert np.array_equal(got, p.prefix())
            continue
        assert getattr(o, f) == w, (name, f)
    # every option left alone is 0: the library's defaults
    for f in names:
        if name == "defaults" and f != "lsd_steps":
            assert not getattr(o, f), f
    assert GenerationParams().slot_opts().lsd_steps == 0  # no default named: the engine's cap
    # the five layouts, filled the old way, hold the same values in every field they have
    for K in (SlotOpts, SlotOpts2, SlotOpts3, SlotOpts4, SlotOpts5):
        old = (K * 1)(K(C.sizeof(K), *want[:len(K._fields_) - 1]))[0]
        assert old.size == C.sizeof(K)
        for f, _ in K._fields_[1:]:
            if f == "prefix_latents":
                assert (old.prefix_latents is None) == (o.prefix_latents is None)
            else:
                assert getattr(old, f) == getattr(o, f), (name, K.__name__, f)
