"""CPU: the dispatcher's "four failures in a row" rule (manga_ocr/multi.py) must not drop a healthy child over ONE bad crop.

tests/test_multi_dispatch.py's cursed-crop case leaves to the scheduler which child is dealt the bad half of a halved chunk; here
the order is forced.  The bad crop is the LAST row of child 1's first chunk, so after every halving it lies in the right half,
which goes to child 1 whenever child 0 - first in the dealing order - is idle and takes the left one.  Child 0 is idle every
time: it answers at once, while child 1 takes a moment to fail.  So child 1 meets the bad crop four times running - its own
chunk [8, 16), then [12, 16), [14, 16), [15, 16) - with no success in between, although nothing is wrong with it: only the
first of the four is a FRESH chunk, the others are pieces of a chunk that had already failed on both children."""
import time

import numpy as np
import pytest

from manga_ocr.multi import MultiGpuEngine, ShardError
from test_multi_dispatch import FakeEngine, _crops, _want


class SlowToFail(FakeEngine):
    """child 1 needs a moment before it raises on the cursed crop; everything else answers at once"""

    def recognize_images(self, images, bgr=False):
        if self.rank == 1 and any(im.shape[0] == 13 for im in images):
            time.sleep(0.15)
        return super().recognize_images(images, bgr)


def slow_factory(rank, device, args):
    return SlowToFail(rank, args)


def test_one_bad_crop_met_four_times_running_costs_no_child():
    crops = _crops(3, 16)
    crops[15] = np.zeros((13, 20), np.uint8)
    eng = MultiGpuEngine([0, 1], factory=slow_factory, backend="gloo", min_chunk=8, max_chunk=8)
    try:
        with pytest.raises(ShardError, match="cursed") as ei:
            eng.recognize_images(crops)
        e = ei.value
        assert sorted(e.failed) == [15] and "worker 1" in e.failed[15], "the forced order: child 1 met the bad crop last, alone"
        good = list(range(15))
        np.testing.assert_array_equal(e.ids[good], _want(crops[:15])[0])
        assert eng.stats["redealt"] == 5 and eng.stats["chunks"][1] == 4, "child 1 was dealt its chunk and the three bad pieces"
        assert eng.alive == [0, 1] and not eng.stats["lost"], "a chunk that has failed before counts against nobody"
        ids, _ = eng.recognize_images(crops[:4])
        np.testing.assert_array_equal(ids, _want(crops[:4])[0])
        assert eng.stats["mode"] == "allgather"
    finally:
        eng.close()
