"""Fitness vectors for populations that need more than one tile of the ranking kernels (es_rank_kernel / es_rank_q_kernel in
csrc/bsk_es.hip stage the fitness through LDS 256 values at a time, one workgroup per 256 members), shared by the GPU tests of the
evolution strategy.  TEST CODE.

The awkward values sit where the tile boundary can matter: a member's rank counts the members of EVERY tile that beat it, and among
equal values - and among NaNs - the lower index wins, which the kernel can only get right from the index base + t of a staged
value.  P = 258 leaves the last tile and the second workgroup exactly one pair, so the cases are spread over several vectors.
"""
import json
import os

import numpy as np

TILE = 256

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "es_tail_seeds.json")) as _fh:
    _TAIL = json.load(_fh)
# the far branch of the inverse normal CDF (r > 5) is min(k, 2^52 - 1 - k) <= TAIL_K_FAR
TAIL_K_FAR = int(_TAIL["k_far"])


def tail_rows():
    """tests/golden/es_tail_seeds.json -> [(seed, j, k, z), ...]: seeds under which z(g = 0, pair 0, j) comes from the far tail
    (tools/es_tail_seeds.c found them), k the 52-bit integer behind the draw and z the float64 the restatement gives, recorded as
    ``float.hex()``"""
    return [(int(r["seed"]), int(r["j"]), int(r["k"]), float.fromhex(r["z"])) for r in _TAIL["rows"]]


def beyond_one_tile(n_members, rng):
    """-> a list of (n_members,) float64 vectors, empty up to one tile.  ``last`` being the first member of the last tile:
      0  an exact tie between member 5 and member last + 1 (tiles 0 and 2 at P = 600) and a single NaN at ``last``; from 302 members
         on also a tie between members 7 and 300 (tiles 0 and 1) and one between 255 and 256, either side of the first boundary
      1  a NaN pair at (256, 257), and a NaN at 11 for it to tie with across the boundary
      2  an exact tie between the two first members of the last tile, which is also the greatest value there is
      3  +inf and -inf at (last, last + 1); +inf a second time at 40"""
    if n_members <= TILE:
        return []
    last = TILE * ((n_members - 1) // TILE)
    a, b, c, d = (rng.normal(size=n_members) for _ in range(4))
    a[last + 1], a[last] = a[5], np.nan
    if n_members >= 302:
        a[300], a[256] = a[7], a[255]
    b[256] = b[257] = b[11] = np.nan
    c[last] = c[last + 1] = np.abs(c).max() + 1.0
    d[last], d[last + 1], d[40] = np.inf, -np.inf, np.inf
    return [a, b, c, d]
