"""The FlowLM step attention (attention_step_qkv, kind C of test_gpu_attention_core) on the paths
its load order separates: the first key block is requested branch-free at kernel entry together
with the QKV slabs and the RoPE row, each key's base (the voice's shared prefix below F, the slot's
own rows from F on) is chosen per element, the slab loop has a fixed trip count with clamped
addresses, and a wave without keys yet still requests (and drops) position 0. A wrong base, a wrong
clamp or a slab counted twice changes the output far beyond the gate: V rows are distinct per
position and differ between the prefix and the store, and the slabs are random.

nh = 2, cap = 160, three slots per launch, 1 / 4 / 8 slabs (the kernel instances unrolled to 8
slabs; test_gpu_attention_core runs 16), with and without prefix tables (the two first-block
policies). Every case is checked in the two layers of test_gpu_attention_core with its bounds
(run_case: RoPE / append gate, the untouched store bit-equal, O against the fp64 attention)."""

import pytest
from test_gpu_attention_core import C, c_layout, eng, run_case  # noqa: F401  (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu

CAP, NH = 160, 2
# name -> (positions of the three slots, prefix lengths or None)
CASES = {
    # no prefix tables at all (F = 0): the non-temporal first block; a wave with no keys (qp 1: waves 1-3)
    "nopre": ((1, 40, 100), None),
    # prefix tables with F = 0 on every slot: the select always takes the slot's own rows
    "pre0": ((1, 40, 100), [0, 0, 0]),
    # F = 5 at position 5: every cached key is a prefix key, the new key the slot's first own row
    "pre5_at5": ((5, 5, 5), [5, 5, 5]),
    # F = 33 at position 70: wave 1's block (keys 32 .. 63) straddles the prefix end; 69 and 71 beside it
    "pre33_at70": ((70, 69, 71), [33, 33, 33]),
    # the round boundary (128 keys per round): the second round has 0 or 1 key
    "round": ((127, 128, 129), None),
    "round_pre": ((127, 128, 129), [33, 0, 130]),
    # the last position, a finished row that filled its cache (appends nothing), a short row beside them
    "cap": ((CAP - 1, CAP, 10), None),
    "cap_pre": ((CAP - 1, CAP, 10), [33, 160, 5]),
}
FAMILIES = ["s5", "spike_first", "spike_last", "spike_new", "spike_pre_last", "spike_own_first"]


@pytest.mark.parametrize("splits", [0, 1, 4, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_step_attention_load_paths_match_fp64(eng, case, splits):  # noqa: F811
    import pocket_tts_amd as pt

    qps, pre = CASES[case]
    lay = c_layout(f"{case}_S{splits}", qps, splits, pre=pre, cap=CAP, nh=NH)
    if splits == 0:
        # dense rows: the step launcher has no such form (its QKV always arrives as split-K slabs);
        # the hook refuses the call instead of launching on them
        with pytest.raises(pt.PocketTTSError, match="takes slabs"):
            run_case(eng, C, lay, "s5", 1)
        return
    worst_r = worst_o = 0.0
    for i, family in enumerate(FAMILIES):
        r, o, _, out, kv1 = run_case(eng, C, lay, family, 7000 + 31 * i + splits)
        worst_r, worst_o = max(worst_r, r), max(worst_o, o)
    print(f"{lay.name}: worst RoPE err/gate {worst_r:.3g}, worst O err/gate {worst_o:.3g}")
