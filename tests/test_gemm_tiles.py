"""CPU: the product library's GEMM tile table (ptts_gemm_tiles, csrc/kernels.h PTTS_TILES) against
the tile lists of tests/test_gpu_gemm_core.py, so every shipped tile has its fp64 test and every
tested tile is shipped."""

import test_gpu_gemm_core as core


def tiles():
    from pocket_tts_amd import Engine

    return Engine.gemm_tiles()


def test_every_shipped_tile_is_tested_and_every_tested_tile_is_shipped():
    ids = [t["id"] for t in tiles()]
    assert len(ids) == len(set(ids)), ids
    listed = core.F32_LAYOUTS + core.BF16_LAYOUTS + core.X6_LAYOUTS
    assert len(listed) == len(set(listed)), listed
    assert set(ids) == set(listed), (sorted(set(ids) - set(listed)), sorted(set(listed) - set(ids)))
    by_ops = {ops: sorted(t["id"] for t in tiles() if t["operands"] == ops) for ops in ("f32", "bf16", "bf16x6")}
    assert by_ops == {"f32": sorted(core.F32_LAYOUTS), "bf16": sorted(core.BF16_LAYOUTS),
                      "bf16x6": sorted(core.X6_LAYOUTS)}


def test_rows_are_consistent():
    for t in tiles():
        assert t["tm"] % 32 == 0 and t["tn"] % 32 == 0 and t["bk"] in (32, 64), t
        # a twin (+ 100 bf16, + 200 bf16x6) has its f32 tile's shape
        assert t["operands"] == {0: "f32", 1: "bf16", 2: "bf16x6"}[t["id"] // 100], t
    # every split-K case of the GPU test runs K = 640 in 3 slabs on BK-32 tiles
    by_id = {t["id"]: t for t in tiles()}
    split_k = [m for m in core.test_split_k_slabs_sum_to_product.pytestmark if m.name == "parametrize"][0].args[1]
    assert all(by_id[i]["bk"] == 32 for i in split_k)


def test_split_tail_set():
    """The tail-capable tiles are the interleaved-DMA f32 tiles: 34 and 35 (the prefill's), and 32
    (the back part's, which the engine runs without a tail). The GPU test's cases lie inside."""
    tail = {t["id"] for t in tiles() if t["tail"]}
    assert {34, 35} <= tail and tail == {32, 34, 35}, tail
    assert all(t["operands"] == "f32" for t in tiles() if t["tail"])
    cases = [m for m in core.test_split_tail_matches_fp64.pytestmark if m.name == "parametrize"][0].args[1]
    assert {c[0] for c in cases} <= tail
    assert 6 not in tail  # test_gpu_gemm_core.test_tail_on_a_tile_without_it_is_refused
