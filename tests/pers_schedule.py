"""The schedules of the persistent encoder GEMM (csrc/kernels_gemm_pers.h) restated in Python: the strip schedule as the
kernel derives it from blockIdx.x (host mirror pers_strip_rows / pers_strip_wins in csrc/engine.hip), the classes of strips
and tiles a shape reaches, and the tile order in column groups (gemm_tile_of, csrc/kernels_gemm.h).  Shared by
tests/test_strip_schedule.py, tests/test_pers_schedule_cpu.py and tests/test_gpu_encoder_gemm.py."""
import numpy as np


def strip_blocks(M, ntn, grid):
    """-> list of (block, col, [(m0, lo, hi, half), ...]) exactly as the kernel derives them from blockIdx.x."""
    out = []
    slots = grid >> 3
    spx = slots // ntn
    used = spx * ntn
    nstrips = 8 * spx + (8 * (slots - used)) // ntn
    for b in range(grid):
        xcd, k = b & 7, b >> 3
        if k < used:
            strip, col = xcd * spx + k // ntn, k % ntn
        else:
            j = (k - used) * 8 + xcd
            strip, col = 8 * spx + j // ntn, j % ntn
        if strip >= nstrips:
            continue
        U = (M + 15) >> 4
        base, extra = U // nstrips, U % nstrips
        u0 = strip * base + min(strip, extra)
        nu = base + (1 if strip < extra else 0)
        rs, re = u0 * 16, min(M, (u0 + nu) * 16)
        if re <= rs:
            continue
        R = re - rs
        rem = R & 255
        ntl = (R >> 8) + (1 if rem else 0)
        hpos = -1
        if rem and rem <= 128:
            v = strip % 3
            hpos = ntl - 1 if v == 0 else 0 if v == 1 else ntl >> 1
        tiles = []
        for t in range(ntl):
            half = t == hpos
            lo = rs + 256 * t - ((256 - rem) if (hpos >= 0 and t > hpos) else 0)
            hi = min(re, lo + (rem if half else 256))
            m0 = max(0, min(lo, hi - (128 if half else 256)))
            tiles.append((m0, lo, hi, half))
        out.append((b, col, tiles))
    return out


def strip_grid(M, N, blocks, cus=256):
    """the grid launch_gemm_pers gives the kernel: `blocks` (0: one per compute unit), at most one per tile, a multiple of 8"""
    ntiles = -(-M // 256) * (N // 256)
    return max(8, min(blocks or cus, (ntiles + 7) // 8 * 8) // 8 * 8)


STRIP_CLASSES = ("half first", "half middle", "half last", "half exactly 128", "one half tile", "one short tile", "clamped to row 0",
                 "short shifted", "whole tiles only", "in-XCD strip", "left-over strip", "idle block", "M not a multiple of 16")


def strip_classes(M, ntn, grid):
    """the names of STRIP_CLASSES a launch of the strip schedule reaches"""
    blocks = strip_blocks(M, ntn, grid)
    used = ((grid >> 3) // ntn) * ntn
    got = set()
    if len(blocks) < grid:
        got.add("idle block")
    if M % 16:
        got.add("M not a multiple of 16")
    for b, _, tiles in blocks:
        got.add("in-XCD strip" if (b >> 3) < used else "left-over strip")
        n = len(tiles)
        if all(hi - lo == 256 and not half for _, lo, hi, half in tiles):
            got.add("whole tiles only")
        for t, (m0, lo, hi, half) in enumerate(tiles):
            if half:
                if n == 1:
                    got.add("one half tile")
                else:
                    got.add("half first" if t == 0 else "half last" if t == n - 1 else "half middle")
                if hi - lo == 128:
                    got.add("half exactly 128")
            elif hi - lo < 256:
                if n == 1:
                    got.add("one short tile")
                    if lo == 0 and hi - 256 < 0:
                        got.add("clamped to row 0")       # the window cannot end with the tile's last row: it starts at row 0
                if m0 < lo:
                    got.add("short shifted")              # the window starts above the tile's own rows
    return got


# (tile code, M, N) -> the classes the GPU test means to run there.  4100: the strip schedule on 8 blocks, 4099: on one block per
# compute unit (at most one per tile).  tests/test_pers_schedule_cpu.py asserts the classes, tests/test_gpu_encoder_gemm.py runs
# the shapes.
STRIP_SHAPES = {
    (4100, 4736, 256): {"half last", "half first", "half middle"},
    (4100, 3200, 256): {"short shifted"},
    (4100, 4096, 256): {"whole tiles only"},
    (4100, 896, 256): {"one half tile"},
    (4100, 1664, 256): {"one short tile", "clamped to row 0"},
    (4100, 1250, 768): {"left-over strip", "idle block", "M not a multiple of 16", "half exactly 128"},
    (4100, 1000, 1024): {"left-over strip", "whole tiles only", "short shifted"},
    (4099, 2200, 768): {"in-XCD strip", "left-over strip", "idle block"},
    (4099, 1000, 1024): {"left-over strip", "one short tile", "short shifted"},      # four strips of 240 .. 256 rows, no XCD holds one
}
STRIP_GRIDS = {(4099, 2200, 768): 32, (4099, 1000, 1024): 16}


def strip_wins(M, ntn, grid):
    """pers_strip_wins: the rounds of 256 x 256 tiles the slowest block walks, tile list against strips (a half tile ~0.6 of a tile)"""
    ntiles = -(-M // 256) * ntn
    if ntiles < 2 * grid:
        return False
    chunk = (ntiles + 7) // 8
    per_block = -(-chunk // (grid >> 3))
    slots = grid >> 3
    nstrips = 8 * (slots // ntn) + (8 * (slots - (slots // ntn) * ntn)) // ntn
    if nstrips <= 0:
        return False
    R = -(-((M + 15) >> 4) // nstrips) * 16
    rem = R & 255
    cost = (R >> 8) + (0.0 if rem == 0 else 0.6 if rem <= 128 else 1.0)
    return cost <= 0.965 * per_block


def tile_of(bid, ntm, ntn, group_n):
    """gemm_tile_of: linear tile id (a numpy array or an int) -> (tm, tn), column group by column group"""
    bid = np.asarray(bid)
    gn = group_n if 0 < group_n < ntn else ntn
    per_group = ntm * gn
    ngroups = (ntn + gn - 1) // gn
    g = np.minimum(bid // per_group, ngroups - 1)
    r = bid - g * per_group
    gw = np.minimum(gn, ntn - g * gn)
    tm = r // gw
    tn = g * gn + r - tm * gw
    return tm, tn
