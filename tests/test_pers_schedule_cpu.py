"""CPU: what tests/test_gpu_encoder_gemm.py relies on without a device - the shapes it gives the strip schedule reach every
class of strip and tile the kernel distinguishes (tests/pers_schedule.py restates the kernel's arithmetic), and the tile order
in column groups (gemm_tile_of) names every tile exactly once whatever the group size."""
import numpy as np

from pers_schedule import STRIP_CLASSES, STRIP_GRIDS, STRIP_SHAPES, strip_classes, strip_grid, strip_wins, tile_of


def test_the_strip_shapes_reach_every_class():
    reached = set()
    for (code, M, N), want in STRIP_SHAPES.items():
        grid = strip_grid(M, N, 8 if code == 4100 else 0)
        assert grid == STRIP_GRIDS.get((code, M, N), 8), (code, M, N, grid)
        got = strip_classes(M, N // 256, grid)
        assert want <= got, f"{code} {M} x {N} on {grid} blocks reaches {sorted(got)}, not {sorted(want - got)}"
        reached |= got
    assert reached == set(STRIP_CLASSES), set(STRIP_CLASSES) - reached
    # the 8-block shapes with one column slice own no left-over blocks: their eight strips are the eight XCDs' own
    assert "left-over strip" not in strip_classes(4736, 1, 8) and "idle block" not in strip_classes(4736, 1, 8)


def test_tile_order_is_a_bijection_onto_the_tiles():
    """every (tm, tn) exactly once for ntm <= 40, ntn <= 13 and group sizes 0 .. 14 (0 and >= ntn: one group; a last group
    narrower than the others), and inside a group the order is M-major / N-minor"""
    for ntm in range(1, 41):
        for ntn in range(1, 14):
            bid = np.arange(ntm * ntn)
            for gn in range(0, 15):
                tm, tn = tile_of(bid, ntm, ntn, gn)
                assert tm.min() >= 0 and tm.max() < ntm and tn.min() >= 0 and tn.max() < ntn, (ntm, ntn, gn)
                assert np.unique(tm * ntn + tn).size == ntm * ntn, f"ntm {ntm} ntn {ntn} group_n {gn}: a tile is named twice"
    # the encoder's own orders: QKV 9 N-tiles in groups 6 + 3, FC1 12 in 6 + 6
    tm, tn = tile_of(np.arange(2 * 9), 2, 9, 6)
    assert tn.tolist() == [0, 1, 2, 3, 4, 5] * 2 + [6, 7, 8] * 2 and tm.tolist() == [0] * 6 + [1] * 6 + [0] * 3 + [1] * 3
    tm, tn = tile_of(np.arange(12), 1, 12, 6)
    assert tn.tolist() == list(range(12))


def test_the_products_choice_of_schedule_at_the_encoder_shapes():
    """pers_strip_wins restated: batch 256 (50,432 rows, N = 768: 591 tiles, three rounds against strips of two tiles and a half
    tile) takes strips on 256 blocks, 8,900 rows (105 tiles on 112 blocks: not two per block) the tile list"""
    assert strip_wins(50432, 3, 256) and not strip_wins(8900, 3, strip_grid(8900, 768, 0))
    assert strip_grid(8900, 768, 0) == 112
