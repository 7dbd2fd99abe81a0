"""The seeded inputs of tests/test_align_kernels_gpu.py, kept apart from it so that tests/test_align_ref_cpu.py can check every
row's margin without a device.  The kernels' block sizes are 64 (columns per step of a wave) and 256 (frames per step of the
entry pass); a workgroup of the row pass holds 4 rows."""
import collections

import numpy as np

import align_ref as R

Case = collections.namedtuple("Case", "B N T_in f16 ld_pad in_len out_len seed")

T_INS = (1, 63, 64, 65, 257)
NS = (1, 2, 255, 256, 257, 1000)


def _lens(B, hi, seed, extra):
    """B ragged lengths in [1, hi] with `extra` (0, values beyond hi, negatives) put in front where the batch has room"""
    rng = np.random.RandomState(seed)
    v = [int(x) for x in rng.randint(1, hi + 1, B)]
    v[-1] = hi
    for i, e in enumerate(extra[:max(0, B - 1)]):
        v[i] = e
    return v


def _cases():
    out = []
    for i, T in enumerate(T_INS):
        for j, N in enumerate(NS):
            B = 3 if N <= 257 else 2
            seed = 100 * i + j
            # every T_in and every N meets both source kinds; rows are 0, 3 or 8 elements wider than T_in
            out.append(Case(B, N, T, (i + j) % 2 == 1, (0, 3, 8)[(i + 2 * j) % 3], _lens(B, T, seed, [T + 5, 0][:(i + j) % 3]),
                            _lens(B, N, seed + 50, [0, N + 9][:(i + j + 1) % 3]), seed))
    # no lengths at all, and one of the two
    out.append(Case(2, 257, 65, False, 0, None, None, 900))
    out.append(Case(2, 300, 63, True, 1, None, [300, 17], 901))
    out.append(Case(2, 300, 64, False, 0, [64, 9], None, 902))
    # more than four rows' worth of entries behind each other: B N no multiple of 4
    out.append(Case(5, 7, 130, True, 2, [130, 1, 64, 65, 129], [7, 0, 3, 7, 1], 903))
    return out


CASES = _cases()


def make(c, path=None):
    """the case's alignments, [B, N, T_in] float32 or float16: clean values everywhere (the GPU test poisons what lies behind the
    lengths)"""
    return R.random_alignments(c.B, c.N, c.T_in, np.float16 if c.f16 else np.float32, c.seed, c.in_len, path)


def edge_cases():
    """Paths laid over the edges of the entry pass's 256-frame blocks -> [(name, Case, path [1, N], {stats field: its value})]:
    a stall run across frame 255 | 256, one across two edges, the largest skip exactly between 255 and 256, the largest backward
    step exactly between 511 and 512.  Elsewhere the path advances by one symbol every 12 frames."""
    N, T = 600, 65
    t = np.arange(N)
    out = []
    p = np.where(t < 250, t // 12, np.where(t < 263, 21, 22 + (t - 263) // 12))
    out.append(("a stall of 13 across frame 256", p, {2: 1, 3: 0, 4: 13}))
    p = np.where(t < 200, t // 40, np.where(t < 531, 5, 6 + (t - 531) // 12))
    out.append(("a stall of 331 across two edges", p, {2: 1, 3: 0, 4: 331}))
    p = np.where(t < 256, t // 12, 28 + (t - 256) // 12)
    out.append(("a skip of 7 from frame 255 to 256", p, {2: 7, 3: 0, 4: 12}))
    p = np.where(t < 512, t // 12, 33 + (t - 512) // 12)
    out.append(("a backward step of 9 from frame 511 to 512", p, {2: 1, 3: 9, 4: 12}))
    return [(name, Case(1, N, T, k % 2 == 1, k, None, None, 950 + k), path[None].astype(np.int64), want)
            for k, (name, path, want) in enumerate(out)]
