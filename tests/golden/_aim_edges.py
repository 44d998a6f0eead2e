"""What the AIM edge tests share (tests/test_aim_edges_host.py, tests/test_gpu_aim_edges.py): the constants of
csrc/aim.hip the device cases straddle, read from the sources; a Python copy of its ``hash32``; tables whose keys are
chosen one by one; and the device-tier cases, each with the constant it is there for.

The numbers below are literals on purpose.  ``test_the_device_cases_sit_on_the_kernels_constants`` fails when a constant
of the kernel moves away from them, so a case cannot quietly stop straddling its seam."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "picasso_amd", "csrc")

# ---- the kernel's constants, as the cases assume them ------------------------------------------------------------------
BLOCK = 256                 # rows_common.h: threads of a block; the LDS init and flush loops step by it
MAX_SHIFTS = 8192           # aim.hip: roi_cc in LDS
GRID_FACTOR = 8             # aim::count: at most GRID_FACTOR * CUs blocks, then the grid-stride loop goes round again
MIN_HSIZE = 1024            # aim::count: the smallest target hash
LOAD_FACTOR = 2             # aim::count: hash slots per target row
DENSE_LIMIT = 1 << 28       # g_dense_limit: target-counter entries of the dense form
HASH_OPS = (("xorshr", 16), ("mul", 0x7feb352d), ("xorshr", 15), ("mul", 0x846ca68b), ("xorshr", 16))

# ---- the device-tier cases, each by the constant it straddles ----------------------------------------------------------
SHIFT_COUNTS = (1, 255, 256, 257, 8192)                   # BLOCK - 1, BLOCK, BLOCK + 1; MAX_SHIFTS (one past it raises)
HASH_SEGMENTS = (10, 600, 10, 600)                        # 2 * 600 > MIN_HSIZE: the hash and the slots grow, then are reused
PARTITION_ROWS = (0, 1, 255, 256, 257, 513)               # BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1: the launch seam
PARTITION_SHAPES = ((100, 1013), (1, 7), (50, 20), (100, 100), (10, 0))          # (seg_len, n_frames)
GRID_TAIL = 257                                           # rows of the second trip: one more than a block


def grid_stride_rows(cu_count):
    """The first row count at which every block of the capped grid has taken its rows and a second trip of GRID_TAIL
    rows is left."""
    return GRID_FACTOR * cu_count * BLOCK + GRID_TAIL


def kernel_constants():
    """The same constants as the sources state them."""
    aim = open(os.path.join(CSRC, "aim.hip")).read()
    rows = open(os.path.join(CSRC, "rows_common.h")).read()

    def one(pattern, text):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0]
    body = one(r"uint32_t hash32\(uint32_t k\)\s*\{(.*?)return k;", aim.replace("\n", " "))
    ops = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        m = re.fullmatch(r"k \^= k >> (\d+)", stmt)
        if m:
            ops.append(("xorshr", int(m.group(1))))
            continue
        m = re.fullmatch(r"k \*= 0x([0-9a-f]+)u", stmt)
        assert m, stmt
        ops.append(("mul", int(m.group(1), 16)))
    grow = re.findall(r"(\d+) \* \(uint64_t\)c\.n", aim)          # the test that regrows and the loop that sizes
    assert len(grow) == 2 and grow[0] == grow[1], grow
    return {
        "BLOCK": int(one(r"constexpr int BLOCK = (\d+);", rows)),
        "MAX_SHIFTS": int(one(r"constexpr int MAX_SHIFTS = (\d+);", aim)),
        "GRID_FACTOR": int(one(r"std::min<int64_t>\(blocks\(c\.n\), (\d+) \* \(int64_t\)device_cu_count\(\)\)", aim)),
        "MIN_HSIZE": int(one(r"uint64_t h = (\d+);", aim)),
        "LOAD_FACTOR": int(grow[0]),
        "DENSE_LIMIT": 1 << int(one(r"g_dense_limit = int64_t\(1\) << (\d+);", aim)),
        "HASH_OPS": tuple(ops),
    }


def hash32(k):
    """csrc/aim.hip hash32 on uint32 values (scalars or arrays)."""
    k = np.asarray(k).astype(np.int64) & 0xFFFFFFFF
    for op, v in HASH_OPS:
        k = (k ^ (k >> v)) if op == "xorshr" else (k * v) & 0xFFFFFFFF
    return k


def keys_hashing_to(slots, hsize, count, start=0):
    """The first `count` int32 keys from `start` on (as signed values) with hash32(key) & (hsize - 1) in `slots`."""
    k = np.arange(start, start + (1 << 22), dtype=np.int64)
    k = k[np.isin(hash32(k) & (hsize - 1), list(slots))][:count]
    assert len(k) == count
    return ((k + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int64)


# ---- tables with chosen keys --------------------------------------------------------------------------------------------
XY_D, XY_W = 1.0, 65536.0                  # x / y: key = x + 65536 y, any int32 from x in [0, 65535], y in [-32768, 32767]
Z_D, Z_W, Z_H = 1.0, 256.0, 256.0          # z: key = x + 256 y + 65536 z, x, y in [0, 255]


def xy_of_keys(k, dtype=np.float64):
    k = np.asarray(k, np.int64)
    return (k & 0xFFFF).astype(dtype), (k >> 16).astype(dtype)


def xyz_of_keys(k, z_dtype=np.float64):
    k = np.asarray(k, np.int64)
    return (k & 0xFF).astype(np.float64), ((k >> 8) & 0xFF).astype(np.float64), (k >> 16).astype(z_dtype)


def hash_case(zmode):
    """Segments of HASH_SEGMENTS rows.  The small ones hold four keys hashing to the last two slots and keys hashing to
    slots 0 and 1, of a table of MIN_HSIZE slots and of the next size alike (the hash has grown by the time the second
    small segment runs), so the probe chains run over the end of the table into slots that are taken as well."""
    big_h = 2 * MIN_HSIZE
    end = keys_hashing_to((big_h - 2, big_h - 1), big_h, 4)
    front = np.concatenate((keys_hashing_to((0,), big_h, 2, start=1), keys_hashing_to((1,), big_h, 2)))
    chain = np.concatenate((end, front))
    assert len(set(chain.tolist())) == 8
    for hsize in (MIN_HSIZE, big_h):
        h = hash32(chain) & (hsize - 1)
        assert (h[:4] >= hsize - 2).all() and sorted(h[4:].tolist()) == [0, 0, 1, 1]
    rng = np.random.default_rng(77)
    others = rng.integers(-2 ** 31, 2 ** 31, 200)
    small_a = np.concatenate((chain, chain[[0, 4]]))
    small_b = np.concatenate((chain[::-1], chain[[1, 7]]))
    big = np.concatenate((chain, chain, others[rng.integers(0, 200, 600 - 16)]))
    big = big[rng.permutation(600)]
    assert (len(small_a), len(big), len(small_b)) == HASH_SEGMENTS[:3]
    assert LOAD_FACTOR * len(small_a) <= MIN_HSIZE < LOAD_FACTOR * len(big) <= big_h
    step = 65536 if zmode else 1
    ref = np.concatenate((chain, chain[:5], chain[:2] + step, chain[2:4] - step, others[:150], others[:40] - step, others[:40]))
    tgt = np.concatenate((small_a, big, small_b))
    segs = [(0, 10), (10, 610), (610, 620), (10, 610)]
    return ref, tgt, segs, step


def partition_restated(frame, seg_len, n_frames):
    """(offsets, per segment the sorted rows) of frames numbered from 1: segment (f - 1) // seg_len over 1 <= f <= n_frames."""
    frame = np.asarray(frame, np.int64)
    n_seg = -(-n_frames // seg_len) if n_frames > 0 else 0
    ok = (frame >= 1) & (frame <= n_frames)
    seg = np.where(ok, (frame - 1) // seg_len, -1)
    sets = [np.flatnonzero(seg == s) for s in range(n_seg)]
    return np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int64), sets


def partition_frames(n, seg_len, n_frames, seed):
    """n unsorted frames: 0, -3, n_frames, n_frames + 1 and 1 first (as many as fit), the others anywhere from -3 to
    n_frames + 1 but in segments 1 and 3, which stay empty where there are more than four."""
    rng = np.random.default_rng(seed)
    n_seg = -(-n_frames // seg_len) if n_frames > 0 else 0
    pool = np.arange(-3, n_frames + 2)
    if n_seg > 4:
        pool = pool[~np.isin((pool - 1) // seg_len, (1, 3)) | (pool < 1) | (pool > n_frames)]
    special = np.array([0, -3, n_frames, n_frames + 1, 1])[:n]
    f = np.concatenate((special, rng.choice(pool, n - len(special)))).astype(np.int64)
    return f[rng.permutation(n)] if n else f
